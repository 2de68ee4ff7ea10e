"""Device-resident ProbabilityGrid and TSDF2D: range-data insertion and
real-time matching without moving the grid across PCIe.

Mirrors what LocalTrajectoryBuilder2D does with the active submap
(``mapping/internal/2d/local_trajectory_builder_2d.cc:78-80, 288-289``):
``ProbabilityGridRangeDataInserter2D::Insert`` (``insert``) and
``RealTimeCorrelativeScanMatcher2D::Match`` (``RealTimeCorrelativeScanMatcher2D.match`` accepts
this class in place of a host ``Grid2D``); ``insert_batch`` makes the insertions of many grids --
both active submaps, or those of many robots -- in one call.  ``TSDF2DOnDevice`` does the same for submaps of
``grid_type = "TSDF"`` with ``TSDFRangeDataInserter2D::Insert``.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Grid2DLimits, TSDFInserterOptions2D, check


class ProbabilityGridOnDevice:
    def __init__(self, resolution, max_xy, num_x_cells, num_y_cells, cells=None, device=0):
        limits = Grid2DLimits(resolution, max_xy[0], max_xy[1], num_x_cells, num_y_cells, 0.0, 0.0)
        self.device = device
        self._h = C.c_void_p()
        ptr = None
        if cells is not None:
            cells = np.ascontiguousarray(cells, np.uint16)
            assert cells.shape == (num_y_cells, num_x_cells)
            ptr = cells.ctypes.data
        check(_lib.lib().cmx_grid2d_create(C.byref(limits), ptr, device, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.lib().cmx_grid2d_destroy(self._h)
            self._h = None

    @property
    def limits(self):
        lim = Grid2DLimits()
        check(_lib.lib().cmx_grid2d_get_limits(self._h, C.byref(lim)))
        return dict(resolution=lim.resolution, max_x=lim.max_x, max_y=lim.max_y,
                    num_x_cells=lim.num_x_cells, num_y_cells=lim.num_y_cells)

    @property
    def cells(self):
        lim = self.limits
        out = np.empty((lim["num_y_cells"], lim["num_x_cells"]), np.uint16)
        check(_lib.lib().cmx_grid2d_download(self._h, out.ctypes.data))
        return out

    def insert(self, origin_xy, returns_xyz, misses_xyz=None, hit_probability=0.7,
               miss_probability=0.4, insert_free_space=True):
        """ProbabilityGridRangeDataInserter2D::Insert + FinishUpdate; points in the map frame."""
        origin = np.ascontiguousarray(origin_xy, np.float32)[:2].copy()
        ret = np.ascontiguousarray(returns_xyz, np.float32).reshape(-1, 3)
        mis = (np.ascontiguousarray(misses_xyz, np.float32).reshape(-1, 3)
               if misses_xyz is not None else np.zeros((0, 3), np.float32))
        check(_lib.lib().cmx_grid2d_insert(
            self._h, origin.ctypes.data, ret.ctypes.data if ret.shape[0] else None, ret.shape[0],
            mis.ctypes.data if mis.shape[0] else None, mis.shape[0], hit_probability,
            miss_probability, int(insert_free_space)))

    def crop(self):
        """grid = grid->ComputeCroppedGrid() (probability_grid.cc:90-106): shrinks the grid to the
        bounding box of its known cells, as Submap2D::Finish does before the loop-closure matcher
        of the submap is built."""
        check(_lib.lib().cmx_grid2d_crop(self._h))

    def fast_matcher(self, branch_and_bound_depth, linear_search_window=7.0,
                     angular_search_window=float(np.deg2rad(30.0))):
        """FastCorrelativeScanMatcher2D of this (finished) grid."""
        from .scan_matching import FastCorrelativeScanMatcher2D
        return FastCorrelativeScanMatcher2D.from_device_grid(
            self, branch_and_bound_depth, linear_search_window, angular_search_window)


def _points(xyz, kept):
    """(pointer or None, count) of an xyz array; the same array object is converted once, so that
    it reaches the library by the same pointer every time it appears in a call."""
    if xyz is None:
        return None, 0
    if id(xyz) not in kept:
        kept[id(xyz)] = (xyz, np.ascontiguousarray(xyz, np.float32).reshape(-1, 3))
    array = kept[id(xyz)][1]
    return (array.ctypes.data if array.shape[0] else None), array.shape[0]


def insert_batch(insertions, hit_probability=0.7, miss_probability=0.4, insert_free_space=True):
    """cmx_grid2d_insert_batch: ``grid.insert(origin_xy, returns_xyz, misses_xyz)`` for every
    ``(ProbabilityGridOnDevice, origin_xy, returns_xyz, misses_xyz_or_None)`` of the list, in list
    order and bit for bit, in shared launches with one synchronisation.  A grid may appear several
    times; an array object passed several times is one scan and is uploaded once."""
    insertions = list(insertions)
    kept = {}                       # id(array) -> (array, float32 copy): alive until the call returns
    items = (_lib.Grid2DInsertion * max(len(insertions), 1))()
    for item, (grid, origin_xy, returns_xyz, misses_xyz) in zip(items, insertions):
        origin = np.ascontiguousarray(origin_xy, np.float32)[:2].copy()
        kept[id(origin)] = (origin, origin)
        item.grid, item.origin_xy = grid._h, origin.ctypes.data
        item.returns_xyz, item.num_returns = _points(returns_xyz, kept)
        item.misses_xyz, item.num_misses = _points(misses_xyz, kept)
    check(_lib.lib().cmx_grid2d_insert_batch(items, len(insertions), hit_probability,
                                             miss_probability, int(insert_free_space)))


def insert_batch_plan(limits, insertions):
    """cmx_debug_grid2d_insert_plan: what one ``insert_batch`` call would do to grids of the given
    limits (dicts with resolution, max_x, max_y, num_x_cells, num_y_cells), without a device.
    ``insertions``: ``(grid index, origin_xy, returns_xyz, misses_xyz_or_None)``.  Returns the round
    of every insertion and the limits of every grid after the call."""
    insertions = list(insertions)
    lims = (Grid2DLimits * len(limits))(*[
        Grid2DLimits(l["resolution"], l["max_x"], l["max_y"], l["num_x_cells"], l["num_y_cells"],
                     0.0, 0.0) for l in limits])
    kept = {}
    items = (_lib.DebugGrid2DInsertion * max(len(insertions), 1))()
    for item, (grid, origin_xy, returns_xyz, misses_xyz) in zip(items, insertions):
        origin = np.ascontiguousarray(origin_xy, np.float32)[:2].copy()
        kept[id(origin)] = (origin, origin)
        item.grid, item.origin_xy = int(grid), origin.ctypes.data
        item.returns_xyz, item.num_returns = _points(returns_xyz, kept)
        item.misses_xyz, item.num_misses = _points(misses_xyz, kept)
    rounds = np.empty(max(len(insertions), 1), np.int32)
    final = (Grid2DLimits * len(limits))()
    check(_lib.lib().cmx_debug_grid2d_insert_plan(lims, len(limits), items, len(insertions),
                                                  rounds.ctypes.data, final))
    return [int(r) for r in rounds[:len(insertions)]], [
        dict(resolution=f.resolution, max_x=f.max_x, max_y=f.max_y, num_x_cells=f.num_x_cells,
             num_y_cells=f.num_y_cells) for f in final]


def _tsdf_options(truncation_distance, maximum_weight, update_free_space, num_normal_samples,
                  sample_radius, project_sdf_distance_to_scan_normal,
                  update_weight_range_exponent, angle_kernel_bandwidth, distance_kernel_bandwidth):
    """cmx_tsdf_inserter_options_2d from the keywords of ``TSDF2DOnDevice.insert``."""
    return TSDFInserterOptions2D(
        truncation_distance, maximum_weight, int(update_free_space), int(num_normal_samples),
        sample_radius, int(project_sdf_distance_to_scan_normal),
        int(update_weight_range_exponent), angle_kernel_bandwidth, distance_kernel_bandwidth)


def _origin_xyz(origin_xyz, kept):
    origin = np.ascontiguousarray(origin_xyz, np.float32).reshape(-1)[:3].copy()
    kept[id(origin)] = (origin, origin)
    return origin.ctypes.data


def tsdf_insert_batch(insertions, **options):
    """cmx_tsdf2d_insert_batch: ``grid.insert(origin_xyz, returns_xyz, **options)`` for every
    ``(TSDF2DOnDevice, origin_xyz, returns_xyz)`` of the list, in list order and bit for bit, in
    shared launches with one synchronisation.  A grid may appear several times; an array object
    passed several times is one scan: it reaches the library by one pointer and, where the origins
    are equal too, is sorted and has its normals estimated once."""
    insertions = list(insertions)
    opts = _tsdf_options(**options)
    kept = {}                       # id(array) -> (array, float32 copy): alive until the call returns
    items = (_lib.TSDF2DInsertion * max(len(insertions), 1))()
    for item, (grid, origin_xyz, returns_xyz) in zip(items, insertions):
        item.grid, item.origin_xyz = grid._h, _origin_xyz(origin_xyz, kept)
        item.returns_xyz, item.num_returns = _points(returns_xyz, kept)
    check(_lib.lib().cmx_tsdf2d_insert_batch(items, len(insertions), C.byref(opts)))


def tsdf_insert_batch_plan(limits, insertions, **options):
    """cmx_debug_tsdf2d_insert_plan: what one ``tsdf_insert_batch`` call would do to grids of the
    given limits (dicts with resolution, max_x, max_y, num_x_cells, num_y_cells), without a
    device.  ``insertions``: ``(grid index, origin_xyz, returns_xyz)``.  Returns, per insertion,
    the round, the limits its grid has at that insertion and the number of rays, and the number of
    distinct scans the call prepares."""
    insertions = list(insertions)
    opts = _tsdf_options(**options)
    lims = (Grid2DLimits * len(limits))(*[
        Grid2DLimits(l["resolution"], l["max_x"], l["max_y"], l["num_x_cells"], l["num_y_cells"],
                     0.0, 0.0) for l in limits])
    kept = {}
    n = len(insertions)
    items = (_lib.DebugTSDF2DInsertion * max(n, 1))()
    for item, (grid, origin_xyz, returns_xyz) in zip(items, insertions):
        item.grid, item.origin_xyz = int(grid), _origin_xyz(origin_xyz, kept)
        item.returns_xyz, item.num_returns = _points(returns_xyz, kept)
    rounds = np.empty(max(n, 1), np.int32)
    rays = np.empty(max(n, 1), np.int32)
    at = (Grid2DLimits * max(n, 1))()
    scans = C.c_int32()
    check(_lib.lib().cmx_debug_tsdf2d_insert_plan(lims, len(limits), items, n, C.byref(opts),
                                                  rounds.ctypes.data, at, rays.ctypes.data,
                                                  C.byref(scans)))
    return ([int(r) for r in rounds[:n]],
            [dict(resolution=f.resolution, max_x=f.max_x, max_y=f.max_y,
                  num_x_cells=f.num_x_cells, num_y_cells=f.num_y_cells) for f in at[:n]],
            [int(r) for r in rays[:n]], int(scans.value))


class TSDF2DOnDevice:
    """TSDF2D(limits, truncation_distance, max_weight) in HBM: the tsd and weight planes (uint16,
    0 = unknown).  The constructor takes the arguments of the test suite's ``ReferenceTSDF2D``;
    ``tsd_cells`` / ``weight_cells`` start it from a copy of two planes instead of all unknown."""

    def __init__(self, resolution, max_xy, num_x_cells, num_y_cells, truncation_distance,
                 max_weight, tsd_cells=None, weight_cells=None, device=0):
        limits = Grid2DLimits(resolution, max_xy[0], max_xy[1], num_x_cells, num_y_cells, 0.0, 0.0)
        self.truncation_distance, self.max_weight = float(truncation_distance), float(max_weight)
        self.device = device
        self._h = C.c_void_p()
        tsd = wgt = None
        if (tsd_cells is None) != (weight_cells is None):
            raise ValueError("give both planes or neither")
        if tsd_cells is not None:
            tsd = np.ascontiguousarray(tsd_cells, np.uint16)
            wgt = np.ascontiguousarray(weight_cells, np.uint16)
            assert tsd.shape == wgt.shape == (num_y_cells, num_x_cells)
        check(_lib.lib().cmx_tsdf2d_create(
            C.byref(limits), truncation_distance, max_weight,
            None if tsd is None else tsd.ctypes.data, None if wgt is None else wgt.ctypes.data,
            device, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.lib().cmx_tsdf2d_destroy(self._h)
            self._h = None

    @property
    def limits(self):
        lim = Grid2DLimits()
        check(_lib.lib().cmx_tsdf2d_get_limits(self._h, C.byref(lim)))
        return dict(resolution=lim.resolution, max_x=lim.max_x, max_y=lim.max_y,
                    num_x_cells=lim.num_x_cells, num_y_cells=lim.num_y_cells)

    def planes(self):
        """(tsd cells, weight cells), uint16 [ny, nx] each."""
        lim = self.limits
        shape = (lim["num_y_cells"], lim["num_x_cells"])
        tsd, wgt = np.empty(shape, np.uint16), np.empty(shape, np.uint16)
        check(_lib.lib().cmx_tsdf2d_download(self._h, tsd.ctypes.data, wgt.ctypes.data))
        return tsd, wgt

    def insert(self, origin_xyz, returns_xyz, truncation_distance, maximum_weight,
               update_free_space, num_normal_samples, sample_radius,
               project_sdf_distance_to_scan_normal, update_weight_range_exponent,
               angle_kernel_bandwidth, distance_kernel_bandwidth):
        """TSDFRangeDataInserter2D::Insert; points in the map frame.  The keywords are those of
        ReferenceTSDF2D.insert, so one dict drives both."""
        origin = np.ascontiguousarray(origin_xyz, np.float32).reshape(-1)[:3].copy()
        ret = np.ascontiguousarray(returns_xyz, np.float32).reshape(-1, 3)
        options = _tsdf_options(
            truncation_distance, maximum_weight, update_free_space, num_normal_samples,
            sample_radius, project_sdf_distance_to_scan_normal, update_weight_range_exponent,
            angle_kernel_bandwidth, distance_kernel_bandwidth)
        check(_lib.lib().cmx_tsdf2d_insert(self._h, origin.ctypes.data,
                                           ret.ctypes.data if ret.shape[0] else None,
                                           ret.shape[0], C.byref(options)))

    def crop(self):
        """grid = grid->ComputeCroppedGrid() (tsdf_2d.cc:118-135)."""
        check(_lib.lib().cmx_tsdf2d_crop(self._h))

    def to_host(self):
        """The planes as a host ``scan_matching.TSDF2D``."""
        from .scan_matching import TSDF2D
        lim = self.limits
        tsd, wgt = self.planes()
        return TSDF2D(tsd, wgt, lim["resolution"], lim["max_x"], lim["max_y"],
                      self.truncation_distance, self.max_weight)

    def fast_matcher(self, branch_and_bound_depth, linear_search_window=7.0,
                     angular_search_window=float(np.deg2rad(30.0))):
        """FastCorrelativeScanMatcher2D of this (finished) grid's tsd plane."""
        from .scan_matching import FastCorrelativeScanMatcher2D
        return FastCorrelativeScanMatcher2D.from_device_grid(
            self, branch_and_bound_depth, linear_search_window, angular_search_window)
