"""Host-side mirror of the reference's point preparation over the C ABI:
``sensor::VoxelFilter`` / ``sensor::AdaptiveVoxelFilter``
(cartographer/sensor/internal/voxel_filter.h:30-45) and
``RotationalScanMatcher::ComputeHistogram``
(cartographer/mapping/internal/3d/scan_matching/rotational_scan_matcher.h:40-42)."""
import ctypes as C

import numpy as np

from . import _lib


def _cloud(point_cloud):
    xyz = np.ascontiguousarray(point_cloud, dtype=np.float32).reshape(-1, 3)
    return xyz, xyz.shape[0]


def voxel_filter(point_cloud, resolution, device=0):
    xyz, n = _cloud(point_cloud)
    out = np.empty((max(n, 1), 3), np.float32)
    kept = C.c_int32()
    _lib.check(_lib.lib().cmx_voxel_filter(xyz.ctypes.data, n, resolution, device,
                                           out.ctypes.data, C.byref(kept)))
    return out[:kept.value].copy()


def voxel_filter_indices(point_cloud, resolution, device=0):
    """Which points ``voxel_filter`` keeps (ascending indices): the overloads of
    ``sensor::VoxelFilter`` over timed points / range measurements
    (cartographer/sensor/internal/voxel_filter.cc:154-191) select payload with them."""
    xyz, n = _cloud(point_cloud)
    out = np.empty(max(n, 1), np.int32)
    kept = C.c_int32()
    _lib.check(_lib.lib().cmx_voxel_filter_indices(xyz.ctypes.data, n, resolution, device,
                                                   out.ctypes.data, C.byref(kept)))
    return out[:kept.value].copy()


def adaptive_voxel_filter(point_cloud, max_length, min_num_points, max_range, device=0):
    xyz, n = _cloud(point_cloud)
    out = np.empty((max(n, 1), 3), np.float32)
    kept = C.c_int32()
    _lib.check(_lib.lib().cmx_adaptive_voxel_filter(xyz.ctypes.data, n, max_length,
                                                    min_num_points, max_range, device,
                                                    out.ctypes.data, C.byref(kept)))
    return out[:kept.value].copy()


def adaptive_voxel_filter_indices(point_cloud, max_length, min_num_points, max_range, device=0):
    """Which points ``adaptive_voxel_filter`` keeps (ascending indices into the input): a
    ``sensor::PointCloud`` keeps the intensities of the kept points
    (cartographer/sensor/internal/voxel_filter.cc:138-161,193-198)."""
    xyz, n = _cloud(point_cloud)
    out = np.empty(max(n, 1), np.int32)
    kept = C.c_int32()
    _lib.check(_lib.lib().cmx_adaptive_voxel_filter_indices(xyz.ctypes.data, n, max_length,
                                                            min_num_points, max_range, device,
                                                            out.ctypes.data, C.byref(kept)))
    return out[:kept.value].copy()


def _filter_jobs(jobs):
    """The cmx_filter_job array of `jobs`, the clouds it borrows and the root of every job."""
    items = (_lib.FilterJob * max(len(jobs), 1))()
    clouds, roots = {}, []
    for k, job in enumerate(jobs):
        item = items[k]
        parent = job.get("input_job", -1)
        cloud = job.get("cloud")
        if cloud is not None:
            # the same array object is the same cloud of the call: converted and staged once
            if id(cloud) not in clouds:
                clouds[id(cloud)] = (cloud, _cloud(cloud)[0])
            xyz = clouds[id(cloud)][1]
            item.point_cloud_xyz, item.num_points = xyz.ctypes.data, xyz.shape[0]
        item.input_job = parent
        mode = job.get("mode", "voxel")
        item.mode = {"voxel": _lib.FILTER_VOXEL, "adaptive": _lib.FILTER_ADAPTIVE}.get(mode, mode)
        item.length = job["length"]
        item.min_num_points = job.get("min_num_points", 0.0)
        item.max_range = job.get("max_range", 0.0)
        roots.append(parent if isinstance(parent, int) and 0 <= parent < k else k)
    return items, clouds, roots


def filter_batch(jobs, device=0):
    """Many filters in one call (``cmx_filter_batch``), a filter's output handed to the next on
    the device.  A job is a dict: ``cloud`` (points of a root; the same array object twice is one
    cloud, uploaded once) or ``input_job`` (index of an earlier root: this job filters the points
    that one kept), ``mode`` ("voxel" or "adaptive"), ``length`` (resolution / max_length),
    ``min_num_points`` and ``max_range`` (adaptive), ``indices`` and ``points`` (which outputs are
    wanted, both by default).  Returns per job a dict with ``indices`` (ascending, into the job's
    own input) and ``points``, None where not wanted: what ``voxel_filter(_indices)`` /
    ``adaptive_voxel_filter(_indices)`` return for the job's input."""
    items, clouds, roots = _filter_jobs(jobs)
    outputs = []
    for k, job in enumerate(jobs):
        room = max(items[roots[k]].num_points, 1)
        indices = np.empty(room, np.int32) if job.get("indices", True) else None
        points = np.empty((room, 3), np.float32) if job.get("points", True) else None
        items[k].kept_indices = None if indices is None else indices.ctypes.data
        items[k].filtered_xyz = None if points is None else points.ctypes.data
        outputs.append((indices, points))
    kept = np.zeros(max(len(jobs), 1), np.int32)
    _lib.check(_lib.lib().cmx_filter_batch(items, len(jobs), device, kept.ctypes.data))
    return [dict(indices=None if i is None else i[:n].copy(),
                 points=None if p is None else p[:n].copy())
            for (i, p), n in zip(outputs, kept)]


def filter_batch_plan(jobs):
    """Where the jobs of ``filter_batch(jobs)`` would run (``cmx_debug_filter_batch_plan``; no
    device needed): per job a dict of set, stage, launch, N, lds_bytes, cloud_slot and single,
    and for the call a dict of num_launches, num_sets and staged_bytes."""
    items, clouds, roots = _filter_jobs(jobs)
    wanted = np.zeros(4, np.float32)      # (the plan looks at which outputs are wanted, never into them)
    for k, job in enumerate(jobs):
        items[k].kept_indices = wanted.ctypes.data if job.get("indices", True) else None
        items[k].filtered_xyz = wanted.ctypes.data if job.get("points", True) else None
    plans = (_lib.DebugFilterJobPlan * max(len(jobs), 1))()
    call = _lib.DebugFilterCallPlan()
    _lib.check(_lib.lib().cmx_debug_filter_batch_plan(items, len(jobs), plans, C.byref(call)))
    return ([{name: getattr(plans[k], name) for name, _ in _lib.DebugFilterJobPlan._fields_}
             for k in range(len(jobs))],
            {name: getattr(call, name) for name, _ in _lib.DebugFilterCallPlan._fields_})


def compute_histogram(point_cloud, histogram_size, device=0):
    xyz, n = _cloud(point_cloud)
    out = np.zeros(histogram_size, np.float32)
    _lib.check(_lib.lib().cmx_compute_histogram(xyz.ctypes.data, n, histogram_size, device,
                                                out.ctypes.data))
    return out


def _histogram_jobs(clouds, histogram_size):
    """The cmx_histogram_job array of `clouds`, the converted clouds it borrows and the sizes."""
    sizes = [histogram_size] * len(clouds) if np.isscalar(histogram_size) else list(histogram_size)
    if len(sizes) != len(clouds):
        raise ValueError("histogram_size: an int, or one per cloud")
    items = (_lib.HistogramJob * max(len(clouds), 1))()
    borrowed = {}
    for k, cloud in enumerate(clouds):
        # the same array object is the same cloud of the call: converted and staged once
        if id(cloud) not in borrowed:
            borrowed[id(cloud)] = (cloud, _cloud(cloud)[0])
        xyz = borrowed[id(cloud)][1]
        items[k].point_cloud_xyz, items[k].num_points = xyz.ctypes.data, xyz.shape[0]
        items[k].histogram_size = int(sizes[k])
    return items, borrowed, sizes


def compute_histogram_batch(clouds, histogram_size, device=0):
    """``compute_histogram`` of many clouds in one call (``cmx_compute_histogram_batch``).
    `clouds` is a list of arrays (the same array object twice is one cloud, uploaded once),
    `histogram_size` an int or one per cloud.  Returns a list of float32 arrays: what
    ``compute_histogram(clouds[k], histogram_size[k])`` returns."""
    items, borrowed, sizes = _histogram_jobs(clouds, histogram_size)
    out = [np.zeros(max(int(size), 0), np.float32) for size in sizes]
    for k, histogram in enumerate(out):
        items[k].histogram = histogram.ctypes.data
    _lib.check(_lib.lib().cmx_compute_histogram_batch(items, len(clouds), device))
    return out


def histogram_batch_plan(clouds, histogram_size):
    """Where the jobs of ``compute_histogram_batch(clouds, histogram_size)`` would run
    (``cmx_debug_histogram_batch_plan``; no device needed): per job a dict of route, set, launch,
    slot, N, cloud_slot and lds_bytes, and for the call a dict of staged_bytes, num_launches and
    num_sets."""
    items, borrowed, sizes = _histogram_jobs(clouds, histogram_size)
    wanted = np.zeros(4, np.float32)      # (the plan never looks into the histograms)
    for k in range(len(clouds)):
        items[k].histogram = wanted.ctypes.data
    plans = (_lib.DebugHistogramJobPlan * max(len(clouds), 1))()
    call = _lib.DebugHistogramCallPlan()
    _lib.check(_lib.lib().cmx_debug_histogram_batch_plan(items, len(clouds), plans, C.byref(call)))
    return ([{name: getattr(plans[k], name) for name, _ in _lib.DebugHistogramJobPlan._fields_}
             for k in range(len(clouds))],
            {name: getattr(call, name) for name, _ in _lib.DebugHistogramCallPlan._fields_})
