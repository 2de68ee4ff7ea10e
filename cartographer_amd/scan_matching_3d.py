"""Host-side mirror of the reference's 3D scan-matcher classes over the C ABI
(``cartographer/mapping/internal/3d/scan_matching/real_time_correlative_scan_matcher_3d.h:36-62``
and ``.../fast_correlative_scan_matcher_3d.h:54-137``).

A HybridGrid is handed over as the flattened voxel list its Iterator yields
(numpy structured array ``_lib.VOXEL_DTYPE``); poses are ``Rigid3d`` =
translation + quaternion (w, x, y, z).
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import (Ceres3DOptions, Ceres3DPair, CeresSummary, Fast3DOptions, MatchStats, NodeData3D,
                   Pose3d, Result3D, RtOptions, VOXEL_DTYPE, check)


@dataclass
class Rigid3d:
    translation: tuple = (0.0, 0.0, 0.0)
    rotation: tuple = (1.0, 0.0, 0.0, 0.0)   # w, x, y, z

    def to_c(self):
        p = Pose3d()
        p.t[:] = [float(v) for v in self.translation]
        p.q[:] = [float(v) for v in self.rotation]
        return p

    @staticmethod
    def from_c(p):
        return Rigid3d(tuple(p.t), tuple(p.q))

    def as_array(self):
        return np.array(list(self.translation) + list(self.rotation), np.float64)


def _voxels(v):
    v = np.ascontiguousarray(v, dtype=VOXEL_DTYPE)
    return v, v.shape[0]


def _cloud(point_cloud):
    xyz = np.ascontiguousarray(point_cloud, dtype=np.float32).reshape(-1, 3)
    return xyz, xyz.shape[0]


class RealTimeCorrelativeScanMatcher3D:
    """Match(initial_pose, cloud, hybrid_grid) -> (score, pose)."""

    def __init__(self, linear_search_window, angular_search_window,
                 translation_delta_cost_weight, rotation_delta_cost_weight, device=0):
        self.options = RtOptions(linear_search_window, angular_search_window,
                                 translation_delta_cost_weight, rotation_delta_cost_weight)
        self.device = device
        self.last_stats = None

    def match_grid(self, initial_pose_estimate, point_cloud, grid):
        """``match`` against a HybridGrid that already lives in HBM
        (``grid_3d.HybridGridOnDevice``): only the scan crosses PCIe."""
        xyz, n = _cloud(point_cloud)
        init = initial_pose_estimate.to_c()
        score, pose, stats = C.c_float(), Pose3d(), MatchStats()
        check(_lib.lib().cmx_rt3d_match_grid(C.byref(self.options), grid._h, C.byref(init),
                                             xyz.ctypes.data, n, C.byref(score), C.byref(pose),
                                             C.byref(stats)))
        self.last_stats = stats.as_dict()
        return float(score.value), Rigid3d.from_c(pose)

    def match_grid_batch(self, initial_poses, clouds, grids):
        """``match_grid`` for many (pose, cloud, grid) triples in one call
        (``cmx_rt3d_match_grid_batch``): entry i bit for bit what ``match_grid(initial_poses[i],
        clouds[i], grids[i])`` returns.  The same array object at several places of ``clouds`` is
        one cloud, staged once.  Returns ``(scores, poses, stats)``: float32 scores, a list of
        Rigid3d, the call's summed stats."""
        num = len(grids)
        assert len(initial_poses) == num and len(clouds) == num
        xyz, seen = [], {}
        for c in clouds:
            if id(c) not in seen:
                seen[id(c)] = _cloud(c)[0]
            xyz.append(seen[id(c)])
        handles = (C.c_void_p * num)(*[g._h for g in grids])
        pointers = (C.c_void_p * num)(*[a.ctypes.data for a in xyz])
        counts = np.ascontiguousarray([a.shape[0] for a in xyz], np.int32)
        inits = (Pose3d * num)(*[p.to_c() for p in initial_poses])
        scores = np.zeros(num, np.float32)
        poses = (Pose3d * num)()
        stats = MatchStats()
        check(_lib.lib().cmx_rt3d_match_grid_batch(
            C.byref(self.options), handles, num, C.cast(inits, C.c_void_p), pointers,
            counts.ctypes.data, scores.ctypes.data, C.cast(poses, C.c_void_p), C.byref(stats)))
        self.last_stats = stats.as_dict()
        return scores, [Rigid3d.from_c(p) for p in poses], self.last_stats

    def match(self, initial_pose_estimate, point_cloud, grid_resolution, grid_voxels):
        vox, nv = _voxels(grid_voxels)
        xyz, n = _cloud(point_cloud)
        init = initial_pose_estimate.to_c()
        score = C.c_float()
        pose = Pose3d()
        stats = MatchStats()
        check(_lib.lib().cmx_rt3d_match(C.byref(self.options), grid_resolution, vox.ctypes.data,
                                        nv, C.byref(init), xyz.ctypes.data, n, self.device,
                                        C.byref(score), C.byref(pose), C.byref(stats)))
        self.last_stats = stats.as_dict()
        return float(score.value), Rigid3d.from_c(pose)


class CeresScanMatcher3D:
    """CeresScanMatcher3D (SM3/ceres_scan_matcher_3d.h:48-66).

    ``match(target_translation, initial_pose_estimate, point_clouds_and_hybrid_grids)`` with
    ``point_clouds_and_hybrid_grids = [(point_cloud, grid_resolution, grid_voxels), ...]`` (one
    entry per occupied_space_weight) returns ``(pose_estimate, summary dict)``.  An entry may
    continue with ``intensities, intensity_voxels, (weight, huber_scale, intensity_threshold)``:
    the pair's intensity_hybrid_grid with its IntensityCostFunctionOptions."""

    def __init__(self, occupied_space_weights, translation_weight, rotation_weight,
                 only_optimize_yaw=False, use_nonmonotonic_steps=False, max_num_iterations=12,
                 device=0):
        o = Ceres3DOptions()
        assert 1 <= len(occupied_space_weights) <= 3
        for k, w in enumerate(occupied_space_weights):
            o.occupied_space_weight[k] = float(w)
        o.num_pairs = len(occupied_space_weights)
        o.translation_weight = float(translation_weight)
        o.rotation_weight = float(rotation_weight)
        o.only_optimize_yaw = 1 if only_optimize_yaw else 0
        o.use_nonmonotonic_steps = 1 if use_nonmonotonic_steps else 0
        o.max_num_iterations = int(max_num_iterations)
        self.options = o
        self.device = device

    def match(self, target_translation, initial_pose_estimate, point_clouds_and_hybrid_grids):
        num = self.options.num_pairs
        assert len(point_clouds_and_hybrid_grids) == num
        keep = []
        pairs = (Ceres3DPair * num)()
        for k, entry in enumerate(point_clouds_and_hybrid_grids):
            cloud, resolution, voxels = entry[:3]
            xyz, n = _cloud(cloud)
            vox, nv = _voxels(voxels)
            keep += [xyz, vox]
            pairs[k].point_cloud_xyz = xyz.ctypes.data
            pairs[k].num_points = n
            pairs[k].resolution = float(resolution)
            pairs[k].voxels = vox.ctypes.data if nv else None
            pairs[k].num_voxels = nv
            if len(entry) > 3 and entry[3] is not None:
                # (intensities, intensity voxels, (weight, huber_scale, intensity_threshold)):
                # the pair's intensity_hybrid_grid and its IntensityCostFunctionOptions
                from ._lib import INTENSITY_VOXEL_DTYPE
                ints = np.ascontiguousarray(entry[3], np.float32)
                ivox = np.ascontiguousarray(entry[4], INTENSITY_VOXEL_DTYPE)
                keep += [ints, ivox]
                assert ints.shape[0] == n
                pairs[k].intensities = ints.ctypes.data
                pairs[k].intensity_voxels = ivox.ctypes.data if ivox.shape[0] else None
                pairs[k].num_intensity_voxels = ivox.shape[0]
                pairs[k].intensity_weight = float(entry[5][0])
                pairs[k].intensity_huber_scale = float(entry[5][1])
                pairs[k].intensity_threshold = float(entry[5][2])
        target = np.ascontiguousarray(target_translation, np.float64)
        init = initial_pose_estimate.to_c()
        pose = Pose3d()
        summary = CeresSummary()
        check(_lib.lib().cmx_ceres3d_match(C.byref(self.options), target.ctypes.data, C.byref(init),
                                           C.cast(pairs, C.c_void_p), self.device, C.byref(pose),
                                           C.byref(summary)))
        del keep
        return Rigid3d.from_c(pose), summary.as_dict()

    def match_grids(self, target_translation, initial_pose_estimate, point_clouds_and_grids):
        """``match`` against HybridGrids that already live in HBM
        (``grid_3d.HybridGridOnDevice``): ``[(point_cloud, grid), ...]`` -- what
        LocalTrajectoryBuilder3D::ScanMatch does with the active submap
        (local_trajectory_builder_3d.cc:96-123).  Only the clouds cross PCIe.  An entry may
        continue with ``intensities, intensity_grid, (weight, huber_scale, intensity_threshold)``:
        the pair's resident ``grid_3d.IntensityHybridGridOnDevice``."""
        num = self.options.num_pairs
        assert len(point_clouds_and_grids) == num
        clouds = [_cloud(e[0])[0] for e in point_clouds_and_grids]
        handles = (C.c_void_p * num)(*[e[1]._h for e in point_clouds_and_grids])
        if any(len(e) > 2 and e[2] is not None for e in point_clouds_and_grids):
            from ._lib import Ceres3DIntensityTerm
            terms = (Ceres3DIntensityTerm * num)()
            keep = []
            for k, e in enumerate(point_clouds_and_grids):
                if len(e) <= 2 or e[2] is None:
                    continue
                ints = np.ascontiguousarray(e[2], np.float32)
                assert ints.shape[0] == clouds[k].shape[0]
                keep.append(ints)
                terms[k].grid = e[3]._h
                terms[k].intensities = ints.ctypes.data
                terms[k].weight, terms[k].huber_scale, terms[k].intensity_threshold = \
                    float(e[4][0]), float(e[4][1]), float(e[4][2])
            pointers = (C.c_void_p * num)(*[c.ctypes.data for c in clouds])
            counts = np.ascontiguousarray([c.shape[0] for c in clouds], np.int32)
            target = np.ascontiguousarray(target_translation, np.float64)
            init = initial_pose_estimate.to_c()
            pose = Pose3d()
            summary = CeresSummary()
            check(_lib.lib().cmx_ceres3d_match_grids_intensity(
                C.byref(self.options), target.ctypes.data, C.byref(init), handles, pointers,
                counts.ctypes.data, C.cast(terms, C.c_void_p), C.byref(pose), C.byref(summary)))
            del keep
            return Rigid3d.from_c(pose), summary.as_dict()
        pointers = (C.c_void_p * num)(*[c.ctypes.data for c in clouds])
        counts = np.ascontiguousarray([c.shape[0] for c in clouds], np.int32)
        target = np.ascontiguousarray(target_translation, np.float64)
        init = initial_pose_estimate.to_c()
        pose = Pose3d()
        summary = CeresSummary()
        check(_lib.lib().cmx_ceres3d_match_grids(C.byref(self.options), target.ctypes.data,
                                                 C.byref(init), handles, pointers,
                                                 counts.ctypes.data, C.byref(pose),
                                                 C.byref(summary)))
        return Rigid3d.from_c(pose), summary.as_dict()

    def match_grids_batch(self, target_translations, initial_poses, point_clouds_and_grids):
        """``match_grids`` (without intensity terms) for many trajectories in one upload, launch
        and synchronisation (``cmx_ceres3d_match_grids_batch``): entry i is ``[(point_cloud, grid),
        ...]`` with one pair per occupied_space_weight and is bit for bit what
        ``match_grids(target_translations[i], initial_poses[i], point_clouds_and_grids[i])``
        returns.  The same array object at several places is one cloud, staged once.  Returns
        ``(poses, summaries)``."""
        num, pairs = len(point_clouds_and_grids), self.options.num_pairs
        assert len(target_translations) == num and len(initial_poses) == num
        xyz, seen, handles = [], {}, []
        for entry in point_clouds_and_grids:
            assert len(entry) == pairs
            for cloud, grid in entry:
                if id(cloud) not in seen:
                    seen[id(cloud)] = _cloud(cloud)[0]
                xyz.append(seen[id(cloud)])
                handles.append(grid._h)
        handles = (C.c_void_p * (num * pairs))(*handles)
        pointers = (C.c_void_p * (num * pairs))(*[a.ctypes.data for a in xyz])
        counts = np.ascontiguousarray([a.shape[0] for a in xyz], np.int32)
        targets = np.ascontiguousarray(target_translations, np.float64).reshape(num, 3)
        inits = (Pose3d * num)(*[p.to_c() for p in initial_poses])
        poses = (Pose3d * num)()
        summaries = (CeresSummary * num)()
        check(_lib.lib().cmx_ceres3d_match_grids_batch(
            C.byref(self.options), num, targets.ctypes.data, C.cast(inits, C.c_void_p), handles,
            pointers, counts.ctypes.data, C.cast(poses, C.c_void_p),
            C.cast(summaries, C.c_void_p)))
        return [Rigid3d.from_c(p) for p in poses], [s.as_dict() for s in summaries]

    def refine_batch(self, matchers, found, pose_estimates, constant_data):
        """ConstraintBuilder3D::ComputeConstraint's refinement of a node's search results
        (constraint_builder_3d.cc:263-276): entry i against the high- and low-resolution grids
        ``matchers[i]`` keeps in HBM, one launch.  Returns (poses, summaries); entries with
        ``found[i] == 0`` are passed through."""
        num = len(matchers)
        assert self.options.num_pairs == 2
        handles = (C.c_void_p * num)(*[m._h for m in matchers])
        found = np.ascontiguousarray([1 if f else 0 for f in found], np.int32)
        poses_in = (Pose3d * num)(*[p.to_c() for p in pose_estimates])
        poses_out = (Pose3d * num)()
        summaries = (CeresSummary * num)()
        data = constant_data.to_c()
        check(_lib.lib().cmx_fast3d_refine_batch(
            C.byref(self.options), handles, num, found.ctypes.data, C.cast(poses_in, C.c_void_p),
            C.byref(data), C.cast(poses_out, C.c_void_p), C.cast(summaries, C.c_void_p)))
        return [Rigid3d.from_c(p) for p in poses_out], [s.as_dict() for s in summaries]

    def refine_pairs(self, matchers, found, pose_estimates, constant_datas):
        """``refine_batch`` for pairs that bring their own nodes (the results of
        ``fast3d_match_pairs``): entry i is refined with the clouds of ``constant_datas[i]``, one
        launch.  Entries that are the same ``TrajectoryNodeData`` object are staged once."""
        num = len(matchers)
        assert self.options.num_pairs == 2 and len(constant_datas) == num
        handles = (C.c_void_p * num)(*[m._h for m in matchers])
        found = np.ascontiguousarray([1 if f else 0 for f in found], np.int32)
        poses_in = (Pose3d * num)(*[p.to_c() for p in pose_estimates])
        poses_out = (Pose3d * num)()
        summaries = (CeresSummary * num)()
        pointers, keep = _node_data_pointers(constant_datas)
        check(_lib.lib().cmx_fast3d_refine_pairs(
            C.byref(self.options), handles, num, found.ctypes.data, C.cast(poses_in, C.c_void_p),
            pointers, C.cast(poses_out, C.c_void_p), C.cast(summaries, C.c_void_p)))
        del keep
        return [Rigid3d.from_c(p) for p in poses_out], [s.as_dict() for s in summaries]


def rt3d_batch_plan(matcher, resolutions, num_points, max_point_norms):
    """Where the matches of ``matcher.match_grid_batch`` would run
    (``cmx_debug_rt3d_batch_plan``; needs no grid and no device): per match a dict with the search
    window in steps ``L``, ``A``, its ``T`` translations and ``R`` rotations, the ``route`` (0: the
    segmented exhaustive launches, 1: the single path), the launch ``set`` and the match's
    ``first_block`` and ``blocks`` in it.  ``max_point_norms[i]``: the largest norm of a point of
    cloud i (NaN or infinity: a cloud with a non-finite coordinate)."""
    num = len(resolutions)
    res = np.ascontiguousarray(resolutions, np.float32)
    counts = np.ascontiguousarray(num_points, np.int32)
    norms = np.ascontiguousarray(max_point_norms, np.float32)
    assert counts.shape[0] == num and norms.shape[0] == num
    plans = (_lib.DebugRt3DMatchPlan * num)()
    check(_lib.lib().cmx_debug_rt3d_batch_plan(C.byref(matcher.options), num, res.ctypes.data,
                                               counts.ctypes.data, norms.ctypes.data, plans))
    return [{k: getattr(p, k) for k, _ in p._fields_} for p in plans]


def ceres_match_grids_batch(matcher, target_translations, initial_poses, point_clouds_and_grids):
    """``matcher.match_grids_batch(...)``: the refinement that follows
    ``RealTimeCorrelativeScanMatcher3D.match_grid_batch`` for a fleet, one call."""
    return matcher.match_grids_batch(target_translations, initial_poses, point_clouds_and_grids)


def _node_data_pointers(constant_datas):
    """``const cmx_node_data3d* const*`` for a list of ``TrajectoryNodeData``: one C record per
    distinct object, so that pairs of one node name one pointer.  Returns (array, records)."""
    records = {}
    for data in constant_datas:
        if id(data) not in records:
            records[id(data)] = data.to_c()
    pointers = (C.POINTER(NodeData3D) * len(constant_datas))(
        *[C.pointer(records[id(data)]) for data in constant_datas])
    return pointers, records


@dataclass
class TrajectoryNodeData:
    """TrajectoryNode::Data fields the 3D matcher reads (mapping/trajectory_node.h:45-63)."""
    high_resolution_point_cloud: np.ndarray
    low_resolution_point_cloud: np.ndarray
    rotational_scan_matcher_histogram: np.ndarray
    gravity_alignment: tuple = (1.0, 0.0, 0.0, 0.0)
    _keep: list = field(default_factory=list, repr=False)

    def to_c(self):
        hi, nhi = _cloud(self.high_resolution_point_cloud)
        lo, nlo = _cloud(self.low_resolution_point_cloud)
        hist = np.ascontiguousarray(self.rotational_scan_matcher_histogram, np.float32)
        self._keep[:] = [hi, lo, hist]
        d = NodeData3D()
        d.gravity_alignment[:] = [float(v) for v in self.gravity_alignment]
        d.high_resolution_point_cloud = hi.ctypes.data
        d.num_high_resolution_points = nhi
        d.low_resolution_point_cloud = lo.ctypes.data
        d.num_low_resolution_points = nlo
        d.rotational_scan_matcher_histogram = hist.ctypes.data if hist.size else None
        d.histogram_size = hist.shape[0]
        return d


class FastCorrelativeScanMatcher3D:
    """FastCorrelativeScanMatcher3D(hybrid_grid, low_resolution_grid, histogram, options).

    ``match*`` return a dict (score, pose_estimate, rotational_score,
    low_resolution_score) or None — the reference's ``unique_ptr<Result>``.
    """

    def __init__(self, resolution, voxels, grid_size, low_resolution, low_resolution_voxels,
                 rotational_scan_matcher_histogram, branch_and_bound_depth=8,
                 full_resolution_depth=3, min_rotational_score=0.77,
                 min_low_resolution_score=0.55, linear_xy_search_window=5.0,
                 linear_z_search_window=1.0, angular_search_window=float(np.deg2rad(15.0)),
                 device=0):
        self.options = Fast3DOptions(branch_and_bound_depth, full_resolution_depth,
                                     min_rotational_score, min_low_resolution_score,
                                     linear_xy_search_window, linear_z_search_window,
                                     angular_search_window)
        vox, nv = _voxels(voxels)
        low, nl = _voxels(low_resolution_voxels)
        hist = np.ascontiguousarray(rotational_scan_matcher_histogram, np.float32)
        self.depth = branch_and_bound_depth
        self.last_stats = None
        self._h = C.c_void_p()
        check(_lib.lib().cmx_fast3d_create(C.byref(self.options), resolution, grid_size,
                                           vox.ctypes.data, nv, low_resolution, low.ctypes.data,
                                           nl, hist.ctypes.data if hist.size else None,
                                           hist.shape[0], device, C.byref(self._h)))

    @classmethod
    def from_device_grids(cls, high_grid, low_grid, rotational_scan_matcher_histogram,
                          branch_and_bound_depth=8, full_resolution_depth=3,
                          min_rotational_score=0.77, min_low_resolution_score=0.55,
                          linear_xy_search_window=5.0, linear_z_search_window=1.0,
                          angular_search_window=float(np.deg2rad(15.0))):
        """Matcher of two grids that live in HBM (cartographer_amd.grid_3d.HybridGridOnDevice, on
        one device): resolutions, grid_size and device come from the grids.  The matcher keeps
        its own copies, so the grids may change or go away afterwards."""
        self = cls.__new__(cls)
        self.options = Fast3DOptions(branch_and_bound_depth, full_resolution_depth,
                                     min_rotational_score, min_low_resolution_score,
                                     linear_xy_search_window, linear_z_search_window,
                                     angular_search_window)
        hist = np.ascontiguousarray(rotational_scan_matcher_histogram, np.float32)
        self.depth = branch_and_bound_depth
        self.last_stats = None
        self._h = C.c_void_p()
        check(_lib.lib().cmx_fast3d_create_from_grids(
            C.byref(self.options), high_grid._h, low_grid._h,
            hist.ctypes.data if hist.size else None, hist.shape[0], C.byref(self._h)))
        return self

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.lib().cmx_fast3d_destroy(self._h)
            self._h = None

    def _finish(self, found, result, stats):
        self.last_stats = stats.as_dict()
        if not found.value:
            return None
        return dict(score=float(result.score), pose_estimate=Rigid3d.from_c(result.pose_estimate),
                    rotational_score=float(result.rotational_score),
                    low_resolution_score=float(result.low_resolution_score))

    def match(self, global_node_pose, global_submap_pose, constant_data, min_score):
        node, submap = global_node_pose.to_c(), global_submap_pose.to_c()
        data = constant_data.to_c()
        found, result, stats = C.c_int32(), Result3D(), MatchStats()
        check(_lib.lib().cmx_fast3d_match(self._h, C.byref(node), C.byref(submap), C.byref(data),
                                          min_score, C.byref(found), C.byref(result),
                                          C.byref(stats)))
        return self._finish(found, result, stats)

    def match_full_submap(self, global_node_rotation, global_submap_rotation, constant_data,
                          min_score):
        nq = np.ascontiguousarray(global_node_rotation, np.float64)
        sq = np.ascontiguousarray(global_submap_rotation, np.float64)
        data = constant_data.to_c()
        found, result, stats = C.c_int32(), Result3D(), MatchStats()
        check(_lib.lib().cmx_fast3d_match_full_submap(self._h, nq.ctypes.data, sq.ctypes.data,
                                                      C.byref(data), min_score, C.byref(found),
                                                      C.byref(result), C.byref(stats)))
        return self._finish(found, result, stats)

    def level_box(self, depth):
        """Lowest cell and extent (x, y, z) of one precomputation level's dense array."""
        lo = np.zeros(3, np.int32)
        dims = np.zeros(3, np.int32)
        check(_lib.lib().cmx_fast3d_level_info(self._h, depth, lo.ctypes.data, dims.ctypes.data))
        return lo, dims

    def level(self, depth):
        """Non-zero cells of one precomputation level, int32 [n,4] (x,y,z,value) sorted (z,y,x)."""
        lo, dims = self.level_box(depth)
        cells = np.empty((dims[2], dims[1], dims[0]), np.uint8)
        check(_lib.lib().cmx_fast3d_level_cells(self._h, depth, cells.ctypes.data))
        z, y, x = np.nonzero(cells)
        out = np.stack([x + lo[0], y + lo[1], z + lo[2], cells[z, y, x]], 1).astype(np.int32)
        return out

    def debug_child_sums(self, cells_xyz, wxy, wz, nodes, as_family=False, live_mask=0xff,
                         sums=None, path=None):
        """``cmx_debug_fast3d_child_sums`` (tests): the eight integer child sums of every node of
        ``nodes`` -- int32 [m,4] rows (level, ox, oy, oz) -- over the full-resolution cell indices
        ``cells_xyz`` (int32 [n,3]) of one scan, by the device code of the search.  With
        ``as_family`` the nodes are one family and bit i of ``live_mask`` says whether member i is
        summed.  Returns (sums int32 [m,8], path int32 [m]); ``sums`` / ``path`` given: filled in
        place, the rows of dead members untouched."""
        cells = np.ascontiguousarray(cells_xyz, np.int32).reshape(-1, 3)
        rows = np.ascontiguousarray(nodes, np.int32).reshape(-1, 4)
        c_nodes = (_lib.DebugFast3DNode * max(rows.shape[0], 1))()
        for node, (level, ox, oy, oz) in zip(c_nodes, rows.tolist()):
            node.level, node.ox, node.oy, node.oz = level, ox, oy, oz
        if sums is None:
            sums = np.zeros((rows.shape[0], 8), np.int32)
        if path is None:
            path = np.full(rows.shape[0], -1, np.int32)
        assert sums.dtype == np.int32 and sums.shape == (rows.shape[0], 8) and \
            sums.flags.c_contiguous
        assert path.dtype == np.int32 and path.shape == (rows.shape[0],) and path.flags.c_contiguous
        check(_lib.lib().cmx_debug_fast3d_child_sums(
            self._h, cells.ctypes.data, cells.shape[0], wxy, wz, c_nodes, rows.shape[0],
            1 if as_family else 0, live_mask, sums.ctypes.data, path.ctypes.data))
        return sums, path


def fast3d_create_batch(sources, *, device=0, **options):
    """``cmx_fast3d_create_batch``: the matchers of many submaps in one call (a loaded map, the
    first global constraint of a node against every finished submap).  A source is either the
    tuple of the constructor's arguments ``(resolution, voxels, grid_size, low_resolution,
    low_resolution_voxels, rotational_scan_matcher_histogram)`` or a triple ``(high_grid,
    low_grid, rotational_scan_matcher_histogram)`` of ``grid_3d.HybridGridOnDevice`` resident on
    ``device``; ``options`` are the constructor's keywords and hold for all.  Returns ordinary
    ``FastCorrelativeScanMatcher3D`` objects, each what the constructor / ``from_device_grids``
    builds."""
    sources = list(sources)
    num = len(sources)
    defaults = dict(branch_and_bound_depth=8, full_resolution_depth=3, min_rotational_score=0.77,
                    min_low_resolution_score=0.55, linear_xy_search_window=5.0,
                    linear_z_search_window=1.0, angular_search_window=float(np.deg2rad(15.0)))
    unknown = set(options) - set(defaults)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}")
    defaults.update(options)
    make_options = lambda: Fast3DOptions(*[defaults[k] for k, _ in Fast3DOptions._fields_])  # noqa: E731
    records = (_lib.Fast3DSource * max(num, 1))()
    keep = []                                       # the arrays the records point at
    for k, source in enumerate(sources):
        if len(source) == 3:
            high_grid, low_grid, histogram = source
            records[k].high_resolution_grid = high_grid._h
            records[k].low_resolution_grid = low_grid._h
        else:
            resolution, voxels, grid_size, low_resolution, low_voxels, histogram = source
            vox, nv = _voxels(voxels)
            low, nl = _voxels(low_voxels)
            keep += [vox, low]
            records[k].resolution = resolution
            records[k].grid_size = grid_size
            records[k].voxels = vox.ctypes.data if nv else None
            records[k].num_voxels = nv
            records[k].low_resolution = low_resolution
            records[k].low_resolution_voxels = low.ctypes.data if nl else None
            records[k].num_low_resolution_voxels = nl
        hist = np.ascontiguousarray(histogram, np.float32)
        keep.append(hist)
        records[k].rotational_scan_matcher_histogram = hist.ctypes.data if hist.size else None
        records[k].histogram_size = hist.shape[0]
    handles = (C.c_void_p * max(num, 1))()
    opts = make_options()
    check(_lib.lib().cmx_fast3d_create_batch(C.byref(opts), records, num, device, handles))
    del keep
    matchers = []
    for k in range(num):
        m = FastCorrelativeScanMatcher3D.__new__(FastCorrelativeScanMatcher3D)
        m.options = make_options()
        m.depth = defaults["branch_and_bound_depth"]
        m.last_stats = None
        m._h = C.c_void_p(handles[k])
        matchers.append(m)
    return matchers


def fast3d_match_batch(matchers, node_poses, submap_poses, match_full_submap, min_scores,
                       constant_data):
    """One node's data against many submaps' matchers (ConstraintBuilder3D's fan-out,
    ``constraints/constraint_builder_3d.cc:79-147``) in one call: ``cmx_fast3d_match_batch`` runs
    the pairs concurrently on separate streams.

    ``node_poses[p]`` / ``submap_poses[p]`` are ``Rigid3d`` (only the rotations are read for
    full-submap pairs).  Returns (list of result dicts or None per pair, stats dict).
    """
    num = len(matchers)
    handles = (C.c_void_p * num)(*[m._h for m in matchers])
    nodes = (Pose3d * num)(*[p.to_c() for p in node_poses])
    submaps = (Pose3d * num)(*[p.to_c() for p in submap_poses])
    full = np.ascontiguousarray([1 if f else 0 for f in match_full_submap], np.int32)
    thresholds = np.ascontiguousarray(min_scores, np.float32)
    assert full.shape[0] == num and thresholds.shape[0] == num
    data = constant_data.to_c()
    found = np.zeros(num, np.int32)
    results = (Result3D * num)()
    stats = MatchStats()
    check(_lib.lib().cmx_fast3d_match_batch(
        handles, num, C.cast(nodes, C.c_void_p), C.cast(submaps, C.c_void_p), full.ctypes.data,
        thresholds.ctypes.data, C.byref(data), found.ctypes.data, C.cast(results, C.c_void_p),
        C.byref(stats)))
    out = []
    for p in range(num):
        if not found[p]:
            out.append(None)
            continue
        r = results[p]
        out.append(dict(score=float(r.score), pose_estimate=Rigid3d.from_c(r.pose_estimate),
                        rotational_score=float(r.rotational_score),
                        low_resolution_score=float(r.low_resolution_score)))
    return out, stats.as_dict()


def fast3d_match_pairs(matchers, node_poses, submap_poses, match_full_submap, min_scores,
                       constant_datas):
    """Many nodes against submaps' matchers in one call (``cmx_fast3d_match_pairs``): the burst of
    ``PoseGraph3D::ComputeConstraintsForNode`` when a submap finishes
    (``mapping/internal/3d/pose_graph_3d.cc:370-379``), or several trajectories' nodes against a
    shared set of submaps.  Pair p is ``constant_datas[p]`` against ``matchers[p]``; entries that
    are the same ``TrajectoryNodeData`` object are one node, uploaded once.  Everything else as
    ``fast3d_match_batch``; all matchers live on one device.
    """
    num = len(matchers)
    handles = (C.c_void_p * num)(*[m._h for m in matchers])
    nodes = (Pose3d * num)(*[p.to_c() for p in node_poses])
    submaps = (Pose3d * num)(*[p.to_c() for p in submap_poses])
    full = np.ascontiguousarray([1 if f else 0 for f in match_full_submap], np.int32)
    thresholds = np.ascontiguousarray(min_scores, np.float32)
    assert full.shape[0] == num and thresholds.shape[0] == num and len(constant_datas) == num
    pointers, keep = _node_data_pointers(constant_datas)
    found = np.zeros(num, np.int32)
    results = (Result3D * num)()
    stats = MatchStats()
    check(_lib.lib().cmx_fast3d_match_pairs(
        handles, num, C.cast(nodes, C.c_void_p), C.cast(submaps, C.c_void_p), full.ctypes.data,
        thresholds.ctypes.data, pointers, found.ctypes.data, C.cast(results, C.c_void_p),
        C.byref(stats)))
    del keep
    out = []
    for p in range(num):
        if not found[p]:
            out.append(None)
            continue
        r = results[p]
        out.append(dict(score=float(r.score), pose_estimate=Rigid3d.from_c(r.pose_estimate),
                        rotational_score=float(r.rotational_score),
                        low_resolution_score=float(r.low_resolution_score)))
    return out, stats.as_dict()
