"""FastCorrelativeScanMatcher3D built from hybrid grids resident in HBM
(cmx_fast3d_create_from_grids, FastCorrelativeScanMatcher3D.from_device_grids) against the
voxel-list constructor on what cmx_grid3d_download returns for the same grids: bit-identical
levels, matches and refinements."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

from test_oracle_reference_pins_3d import quat_from_angle_axis

pytestmark = pytest.mark.gpu

SIZE = (9.0, 8.0, 4.0)


@pytest.fixture(scope="module")
def sm3():
    from cartographer_amd import _lib, scan_matching_3d
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching_3d


def _sweep(world, seed, p):
    """Sweep p of synth.make_submap_3d(seed, ...) in the map frame: (origin, returns)."""
    pos = world.free_position(seed * 1009 + p, 0.5)
    yaw = 0.37 * p
    sensor = world.scan(pos, yaw, 10, 128, seed=seed * 31 + p).astype(np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    x = pos[0] + c * sensor[:, 0] - s * sensor[:, 1]
    y = pos[1] + s * sensor[:, 0] + c * sensor[:, 1]
    z = pos[2] + sensor[:, 2]
    return pos.astype(np.float32), np.stack([x, y, z], 1).astype(np.float32)


def _resident_grids(synth, seed, num_sweeps=5, device=0):
    """High (0.10 m) and low (0.45 m) resident grids filled sweep by sweep from positions across
    the room, so both bricks grow several times."""
    from cartographer_amd import grid_3d
    world = synth.World3D(seed, SIZE)
    high = grid_3d.HybridGridOnDevice(0.1, device)
    low = grid_3d.HybridGridOnDevice(0.45, device)
    for p in range(num_sweeps):
        origin, returns = _sweep(world, seed, p)
        high.insert(origin, returns, 0.7, 0.4, 2)
        low.insert(origin, returns, 0.7, 0.4, 2)
    return world, high, low


def _options(depth, frd):
    return dict(branch_and_bound_depth=depth, full_resolution_depth=frd, min_rotational_score=0.9,
                min_low_resolution_score=0.3, linear_xy_search_window=1.5,
                linear_z_search_window=0.5, angular_search_window=math.radians(20.0))


def _histogram(seed):
    rng = np.random.default_rng(seed)
    hist = rng.uniform(0.0, 1.0, 120).astype(np.float32)
    hist[10:14] += 6.0      # a dominant direction: the yaw filter is selective
    return hist


def _pair(sm3, high, low, hist, opt):
    """(A, B): from the resident grids, and from their downloaded voxel lists."""
    a = sm3.FastCorrelativeScanMatcher3D.from_device_grids(high, low, hist, **opt)
    b = sm3.FastCorrelativeScanMatcher3D(0.1, high.voxels(), high.grid_size, 0.45, low.voxels(),
                                         hist, **opt)
    return a, b


def _raw_level(m, depth):
    from cartographer_amd import _lib
    lo = np.zeros(3, np.int32)
    dims = np.zeros(3, np.int32)
    _lib.check(_lib.lib().cmx_fast3d_level_info(m._h, depth, lo.ctypes.data, dims.ctypes.data))
    cells = np.empty((dims[2], dims[1], dims[0]), np.uint8)
    _lib.check(_lib.lib().cmx_fast3d_level_cells(m._h, depth, cells.ctypes.data))
    return lo, dims, cells


def _assert_levels_equal(a, b, depth):
    for d in range(depth):
        la, lb = _raw_level(a, d), _raw_level(b, d)
        np.testing.assert_array_equal(la[0], lb[0], err_msg=f"level {d} lo")
        np.testing.assert_array_equal(la[1], lb[1], err_msg=f"level {d} dims")
        np.testing.assert_array_equal(la[2], lb[2], err_msg=f"level {d} cells")
        np.testing.assert_array_equal(a.level(d), b.level(d), err_msg=f"level {d}")


def _nodes(sm3, world, seed, count=8):
    """`count` nodes: (node pose, submap pose, TrajectoryNodeData).  Some are found, some are not
    (histogram turned the wrong way, threshold above the best score, pose far off)."""
    hist = _histogram(seed)
    submap_pose = [0.3, -0.2, 0.1] + quat_from_angle_axis(0.2, [0, 0, 1])
    c, s = math.cos(0.2), math.sin(0.2)
    out = []
    for k in range(count):
        pos = world.free_position(seed + 3 + k, 0.6)
        yaw = 0.4 + 0.05 * k
        hi = world.scan(pos, yaw, 8, 96, seed=1 + k)
        lo = hi[::7].copy()
        shift = -19 if k % 4 != 3 else 40            # k = 3, 7: the yaw filter rejects
        offset = (0.35, -0.25, 0.1) if k != 5 else (1.2, 1.1, 0.4)
        local = np.array([pos[0] + offset[0], pos[1] + offset[1], pos[2] + offset[2]])
        node_t = [submap_pose[0] + c * local[0] - s * local[1],
                  submap_pose[1] + s * local[0] + c * local[1], submap_pose[2] + local[2]]
        node_pose = node_t + quat_from_angle_axis(0.2 + yaw + 0.1, [0, 0, 1])
        gravity = quat_from_angle_axis(0.01, [1, 0, 0])
        data = sm3.TrajectoryNodeData(hi, lo, np.roll(hist, shift).copy(), tuple(gravity))
        out.append((sm3.Rigid3d(tuple(node_pose[:3]), tuple(node_pose[3:])),
                    sm3.Rigid3d(tuple(submap_pose[:3]), tuple(submap_pose[3:])), data,
                    0.15 if k != 6 else 0.95))
    return out


def _results(sm3, m, nodes, full=True):
    out = []
    for node_pose, submap_pose, data, min_score in nodes:
        out.append(m.match(node_pose, submap_pose, data, min_score))
        if full:
            out.append(m.match_full_submap(node_pose.rotation, submap_pose.rotation, data,
                                           min_score))
    return out


def _key(r):
    if r is None:
        return None
    p = r["pose_estimate"]
    return (np.float32(r["score"]).tobytes(), np.float32(r["rotational_score"]).tobytes(),
            np.float32(r["low_resolution_score"]).tobytes(),
            np.asarray(list(p.translation) + list(p.rotation), np.float64).tobytes())


@pytest.fixture(scope="module")
def scene(synth):
    seed = 21
    world, high, low = _resident_grids(synth, seed)
    return dict(seed=seed, world=world, high=high, low=low, hist=_histogram(seed))


@pytest.mark.parametrize("depth,frd", [(8, 3), (5, 2), (1, 1)])
def test_levels_match_the_voxel_path(sm3, scene, depth, frd):
    a, b = _pair(sm3, scene["high"], scene["low"], scene["hist"], _options(depth, frd))
    _assert_levels_equal(a, b, depth)


@pytest.mark.parametrize("depth,frd", [(8, 3), (5, 2), (1, 1)])
def test_matches_and_refinement_match_the_voxel_path(sm3, scene, depth, frd):
    a, b = _pair(sm3, scene["high"], scene["low"], scene["hist"], _options(depth, frd))
    nodes = _nodes(sm3, scene["world"], scene["seed"])
    ra, rb = _results(sm3, a, nodes), _results(sm3, b, nodes)
    assert [_key(r) for r in ra] == [_key(r) for r in rb]
    found = [r is not None for r in ra]
    assert any(found) and not all(found)
    # The fan-out of one node against several matchers, windowed and full-submap pairs mixed.
    node_pose, submap_pose, data, _ = nodes[0]
    flags = [False, True, False, True]
    batch_a, _ = sm3.fast3d_match_batch([a, a, a, a], [node_pose] * 4, [submap_pose] * 4, flags,
                                        [0.15, 0.15, 0.95, 0.15], data)
    batch_b, _ = sm3.fast3d_match_batch([b, b, b, b], [node_pose] * 4, [submap_pose] * 4, flags,
                                        [0.15, 0.15, 0.95, 0.15], data)
    assert [_key(r) for r in batch_a] == [_key(r) for r in batch_b]
    assert batch_a[0] is not None
    # CeresScanMatcher3D over the raw grids each matcher keeps (cmx_fast3d_refine_batch).
    ceres = sm3.CeresScanMatcher3D([1.0, 6.0], 5.0, 4e2)
    for node_pose, submap_pose, data, min_score in nodes[:4]:
        hit = a.match(node_pose, submap_pose, data, min_score)
        start = hit["pose_estimate"] if hit else node_pose
        pa, sa = ceres.refine_batch([a], [True], [start], data)
        pb, sb = ceres.refine_batch([b], [True], [start], data)
        assert pa == pb and sa == sb


def test_found_case_equals_the_oracle(sm3, oracle, scene):
    opt = _options(6, 3)
    a = sm3.FastCorrelativeScanMatcher3D.from_device_grids(scene["high"], scene["low"],
                                                           scene["hist"], **opt)
    om = oracle.FastCorrelativeScanMatcher3D(
        0.1, scene["high"].voxels(), 0.45, scene["low"].voxels(), scene["hist"], 6, 3, 0.9, 0.3,
        1.5, 0.5, math.radians(20.0))
    node_pose, submap_pose, data, min_score = _nodes(sm3, scene["world"], scene["seed"], 1)[0]
    got = a.match(node_pose, submap_pose, data, min_score)
    ref = om.match(list(node_pose.translation) + list(node_pose.rotation),
                   list(submap_pose.translation) + list(submap_pose.rotation),
                   list(data.gravity_alignment), data.high_resolution_point_cloud,
                   data.low_resolution_point_cloud, data.rotational_scan_matcher_histogram,
                   min_score)
    assert ref["found"] and got is not None
    for key in ("score", "rotational_score", "low_resolution_score"):
        assert np.float32(got[key]) == np.float32(ref[key]), key
    p = got["pose_estimate"]
    np.testing.assert_array_equal(list(p.translation) + list(p.rotation), ref["pose"])


def test_matcher_owns_its_grids(sm3, synth):
    seed = 22
    world, high, low = _resident_grids(synth, seed, num_sweeps=3)
    hist = _histogram(seed)
    opt = _options(8, 3)
    a = sm3.FastCorrelativeScanMatcher3D.from_device_grids(high, low, hist, **opt)
    nodes = _nodes(sm3, world, seed, 4)
    levels = [_raw_level(a, d) for d in range(8)]
    before = [_key(r) for r in _results(sm3, a, nodes)]
    # Insertion that reaches outside both bricks (they are re-allocated), then no grids at all.
    counts = (len(high.voxels()), len(low.voxels()))
    for p in range(3, 6):
        origin, returns = _sweep(world, seed, p)
        high.insert(origin, returns, 0.7, 0.4, 2)
        low.insert(origin, returns, 0.7, 0.4, 2)
    assert len(high.voxels()) > counts[0] and len(low.voxels()) > counts[1]
    del high, low
    gc.collect()
    for d in range(8):
        for x, y in zip(_raw_level(a, d), levels[d]):
            np.testing.assert_array_equal(x, y)
    assert [_key(r) for r in _results(sm3, a, nodes)] == before


def test_empty_grids_behave_like_empty_voxel_lists(sm3, synth):
    from cartographer_amd import grid_3d
    from cartographer_amd._lib import VOXEL_DTYPE
    world, high, low = _resident_grids(synth, 23, num_sweeps=2)
    empty_high, empty_low = grid_3d.HybridGridOnDevice(0.1), grid_3d.HybridGridOnDevice(0.45)
    hist = _histogram(23)
    none = np.zeros(0, VOXEL_DTYPE)
    nodes = _nodes(sm3, world, 23, 2)
    for hi_grid, lo_grid in ((empty_high, empty_low), (empty_high, low), (high, empty_low)):
        for depth, frd in ((8, 3), (1, 1)):
            opt = _options(depth, frd)
            a = sm3.FastCorrelativeScanMatcher3D.from_device_grids(hi_grid, lo_grid, hist, **opt)
            hv = hi_grid.voxels() if hi_grid is high else none
            lv = lo_grid.voxels() if lo_grid is low else none
            b = sm3.FastCorrelativeScanMatcher3D(0.1, hv, hi_grid.grid_size, 0.45, lv, hist,
                                                 **opt)
            _assert_levels_equal(a, b, depth)
            assert [_key(r) for r in _results(sm3, a, nodes)] == \
                [_key(r) for r in _results(sm3, b, nodes)]
    lo0, dims0, cells0 = _raw_level(
        sm3.FastCorrelativeScanMatcher3D.from_device_grids(empty_high, empty_low, hist), 0)
    assert list(lo0) == [0, 0, 0] and list(dims0) == [1, 1, 1] and cells0.sum() == 0


def test_invalid_arguments(sm3):
    from cartographer_amd import _lib, grid_3d
    from cartographer_amd._lib import CmxError, INVALID_ARGUMENT
    L = _lib.lib()
    high, low = grid_3d.HybridGridOnDevice(0.1), grid_3d.HybridGridOnDevice(0.45)
    opts = _lib.Fast3DOptions(8, 3, 0.77, 0.55, 5.0, 1.0, math.radians(15.0))
    h = C.c_void_p()
    hist = np.zeros(4, np.float32)
    calls = [
        (None, high._h, low._h, hist.ctypes.data, 4, C.byref(h)),
        (C.byref(opts), None, low._h, hist.ctypes.data, 4, C.byref(h)),
        (C.byref(opts), high._h, None, hist.ctypes.data, 4, C.byref(h)),
        (C.byref(opts), high._h, low._h, hist.ctypes.data, 4, None),
        (C.byref(opts), high._h, low._h, None, 4, C.byref(h)),
    ]
    for args in calls:
        assert L.cmx_fast3d_create_from_grids(*args) == INVALID_ARGUMENT
        assert not h.value
    for depth, frd in ((0, 1), (13, 1), (4, 0)):      # depth in [1, 12], frd >= 1
        with pytest.raises(CmxError) as e:
            sm3.FastCorrelativeScanMatcher3D.from_device_grids(
                high, low, hist, branch_and_bound_depth=depth, full_resolution_depth=frd)
        assert e.value.status == INVALID_ARGUMENT
    if L.cmx_device_count() > 1:
        other = grid_3d.HybridGridOnDevice(0.45, device=1)
        with pytest.raises(CmxError) as e:
            sm3.FastCorrelativeScanMatcher3D.from_device_grids(high, other, hist)
        assert e.value.status == INVALID_ARGUMENT
