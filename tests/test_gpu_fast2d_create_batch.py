"""cmx_fast2d_create_batch: the matchers of many submaps built by one chain of launches.

Expected values are always the single creates' matchers (cmx_fast2d_create, _from_grid,
_from_tsdf), which the rest of the suite pins to the oracle: every level byte for byte, the
front end's plan, its bounds and lowest-resolution sums, and every result of a search or a
refinement (found flag equal, f32 score bit-equal, pose at atol = 0; of cmx_match_stats only
num_scans and coarse_candidates, which are functions of the inputs).

The six sources of the mixed batch, at depth 5 (w = 16; the plane states are asserted through
cmx_debug_fast2d_plan, from PlanMatcherOf's arithmetic: PI x PJ = ceil((n + 15) / 16) lattice
cells per plane, planes where PI * PJ <= 256, group planes where the stride is 64 and the level
dilated by two cells still fits PI * 16 x PJ * 16):
  0  28 x 28    host cells        PI = PJ = 3, 43 + 4 <= 48: planes and group planes
  1  30 x 30    resident TSDF2D   PI = PJ = 3, 45 + 4 >  48: planes only; cost range [-0.3, 0.3]
  2  120 x 120  host cells        PI = PJ = 9: planes of stride 128
  3  >= 372^2   resident probability grid after inserts and a crop: no planes
  4  1 x 1      host cells        PI = PJ = 1, 16 + 4 > 16: planes only
  5  257 x 63   host cells        17 x 5 lattice cells: planes of stride 128; a row crosses a
                                  256-thread block and the 8 x 4 quad tiles
The two smallest are windows cut out of the 120 x 120 submap: synth.make_submap at that size
leaves all but a handful of cells unknown.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES = 0.05
LIN, ANG = 1.0, math.radians(20.0)
DEPTH = 5
T, W = 0.3, 10.0                        # the TSDF's truncation distance and maximum weight
WITH_SCAN = (2, 3, 5)                   # sources whose world has free space for a scan


@pytest.fixture(scope="module")
def sm():
    from cartographer_amd import _lib, scan_matching
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching


def _xyt(pose):
    return [pose.x, pose.y, pose.theta]


def _in_map(pose, points):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    out = np.array(points, np.float32, copy=True)
    out[:, 0] = pose[0] + c * points[:, 0] - s * points[:, 1]
    out[:, 1] = pose[1] + s * points[:, 0] + c * points[:, 1]
    return out


def _assert_same_result(a, b, what):
    assert a[0] == b[0], what
    if a[0]:
        assert np.float32(a[1]) == np.float32(b[1]), what
        np.testing.assert_allclose(_xyt(a[2]), _xyt(b[2]), rtol=0, atol=0, err_msg=str(what))


def _assert_same_levels(a, b, depth, what):
    for level in range(depth):
        np.testing.assert_array_equal(a.level(level), b.level(level),
                                      err_msg=f"{what}, level {level}")


class Scene:
    """Host data of the six sources, made once; `sources()` makes the grid objects anew (the
    lifetime test destroys them)."""

    def __init__(self, sm, synth, oracle):
        import tsdf_helpers
        self.sm = sm
        mid, lim_mid, world_mid = synth.make_submap(11, 120, 120, RES, 12, 400, 5.0, 0.01)
        big, lim_big, world_big = synth.make_submap(42, 400, 400, RES, 12, 400, 10.0, 0.01)
        wide, lim_wide, world_wide = synth.make_submap(16, 257, 63, RES, 12, 400, 5.0, 0.01)
        self.small = np.ascontiguousarray(mid[46:74, 46:74])
        window = np.ascontiguousarray(mid[40:70, 50:80])
        assert (self.small != 0).sum() > 500 and (window != 0).sum() > 500
        self.tsd, self.wgt = tsdf_helpers.tsdf_from_probability_grid(oracle, window, RES, T, W, 3)
        self.mid, self.lim_mid = mid, lim_mid
        self.big, self.lim_big, self.world_big = big, lim_big, world_big
        self.wide, self.lim_wide = wide, lim_wide
        self.one = np.array([[20000]], np.uint16)
        self.clouds, self.initial = {}, {}
        for k, world, seed in ((2, world_mid, 20), (3, world_big, 31), (5, world_wide, 20)):
            truth = world.free_pose(seed, 0.3)
            scan = world.scan(truth, 300, 5.0, 0.01, k)
            assert len(scan) >= 150
            self.clouds[k] = scan
            self.initial[k] = sm.Rigid2d(float(truth[0] + 0.1), float(truth[1] - 0.05),
                                         float(truth[2] + 0.02))

    def resident_probability_grid(self):
        """The 400 x 400 submap in a larger grid in HBM, four more scans inserted, cropped."""
        from cartographer_amd import grid_2d
        lim = self.lim_big
        padded = np.zeros((430, 420), np.uint16)
        padded[20:420, 10:410] = self.big          # max moved by (1.0, 0.5): 20 rows, 10 columns
        grid = grid_2d.ProbabilityGridOnDevice(RES, (lim["max_x"] + 1.0, lim["max_y"] + 0.5),
                                               420, 430, padded)
        for k in range(4):
            pose = self.world_big.free_pose(30 + k, 0.4)
            grid.insert(pose[:2], _in_map(pose, self.world_big.scan(pose, 300, 10.0, 0.01, k)))
        grid.crop()
        now = grid.limits
        assert (now["num_x_cells"], now["num_y_cells"]) != (420, 430)
        assert now["num_x_cells"] >= 372 and now["num_y_cells"] >= 372
        return grid

    def sources(self):
        from cartographer_amd import grid_2d
        sm = self.sm
        return [
            sm.Grid2D(self.small.copy(), RES, 0.7, 0.7),
            grid_2d.TSDF2DOnDevice(RES, (0.75, 0.75), 30, 30, T, W, self.tsd, self.wgt),
            sm.Grid2D(self.mid.copy(), RES, self.lim_mid["max_x"], self.lim_mid["max_y"]),
            self.resident_probability_grid(),
            sm.Grid2D(self.one.copy(), RES, 0.025, 0.025),
            sm.Grid2D(self.wide.copy(), RES, self.lim_wide["max_x"], self.lim_wide["max_y"]),
        ]

    def single(self, grid, depth):
        sm = self.sm
        if isinstance(grid, sm.Grid2D):
            return sm.FastCorrelativeScanMatcher2D(grid, depth, LIN, ANG)
        return sm.FastCorrelativeScanMatcher2D.from_device_grid(grid, depth, LIN, ANG)

    def batch(self, grids, depth):
        return self.sm.FastCorrelativeScanMatcher2D.create_batch(grids, depth, LIN, ANG)


class Built:
    """The mixed batch at depth 5 next to its single creates, and the single matchers' results
    for the sources with a scan, at a threshold they reach and one they do not."""

    def __init__(self, scene):
        self.grids = scene.sources()
        self.singles = [scene.single(g, DEPTH) for g in self.grids]
        self.batch = scene.batch(self.grids, DEPTH)
        self.thresholds, self.expected = {}, {}
        for k in WITH_SCAN:
            one = self.singles[k]
            cloud = scene.clouds[k]
            best = one.match(scene.initial[k], cloud, 0.0)
            assert best[0]
            self.thresholds[k] = (float(np.float32(best[1] - 0.05)), float(np.float32(best[1] + 0.05)))
            for min_score in self.thresholds[k]:
                windowed = one.match(scene.initial[k], cloud, min_score)
                stats = dict(one.last_stats)
                full = one.match_full_submap(cloud, min_score)
                self.expected[k, min_score] = (windowed, stats, full, dict(one.last_stats))
            assert self.expected[k, self.thresholds[k][0]][0][0]
            assert not self.expected[k, self.thresholds[k][1]][0][0]


@pytest.fixture(scope="module")
def scene(sm, synth, oracle):
    return Scene(sm, synth, oracle)


@pytest.fixture(scope="module")
def built(scene):
    return Built(scene)


def _assert_results_of_c(scene, built, matchers, which):
    """Every matcher of `which` returns what its single create returned."""
    for k in which:
        cloud = scene.clouds[k]
        for min_score in built.thresholds[k]:
            windowed, stats, full, full_stats = built.expected[k, min_score]
            got = matchers[k].match(scene.initial[k], cloud, min_score)
            _assert_same_result(got, windowed, (k, min_score, "match"))
            for name in ("num_scans", "coarse_candidates"):
                assert matchers[k].last_stats[name] == stats[name], (k, min_score, name)
            got = matchers[k].match_full_submap(cloud, min_score)
            _assert_same_result(got, full, (k, min_score, "match_full_submap"))
            for name in ("num_scans", "coarse_candidates"):
                assert matchers[k].last_stats[name] == full_stats[name], (k, min_score, name)


# ---- a. the mixed batch -----------------------------------------------------------------------
def test_mixed_batch_levels_plans_and_front_end(sm, scene, built):
    from cartographer_amd import grid_2d
    assert isinstance(built.grids[1], grid_2d.TSDF2DOnDevice)
    assert isinstance(built.grids[3], grid_2d.ProbabilityGridOnDevice)
    assert len(built.batch) == 6
    for k in range(6):
        _assert_same_levels(built.batch[k], built.singles[k], DEPTH, f"source {k}")
    # The plane states, as the front end's planner reads them off the matchers (every problem a
    # full-submap search of a 300-point cloud reaching 3 m).
    full = [1] * 6
    plan_batch, launch_batch = sm.debug_plan(built.batch, full, num_points=300, max_range_xy=3.0)
    plan_single, launch_single = sm.debug_plan(built.singles, full, num_points=300,
                                               max_range_xy=3.0)
    assert plan_batch == plan_single and launch_batch == launch_single
    states = [(p["use_planes"], p["plane_stride"], p["group"]) for p in plan_batch]
    assert states == [(1, 64, 3),      # planes + group planes
                      (1, 64, 1),      # planes only
                      (1, 128, 1),     # planes of stride 128
                      (0, 0, 1),       # no planes
                      (1, 64, 1),      # planes only (one lattice cell)
                      (1, 128, 1)]     # planes of stride 128
    # windowed searches plan the same way on both
    assert sm.debug_plan(built.batch, [0] * 6, num_points=300, max_range_xy=3.0) == \
        sm.debug_plan(built.singles, [0] * 6, num_points=300, max_range_xy=3.0)
    # Bounds and lowest-resolution sums of the front end, which reads the planes, the group
    # planes and the top level.  The small ones get the 120 x 120 world's scan: what counts is
    # that both matchers see the same bytes.
    for k in range(6):
        cloud = scene.clouds.get(k, scene.clouds[2])
        initial = scene.initial.get(k, sm.Rigid2d(0.3, 0.3, 0.1))
        for full_submap in (False, True):
            a = built.batch[k].debug_prepare(initial, cloud, full_submap)
            b = built.singles[k].debug_prepare(initial, cloud, full_submap)
            assert a["num_scans"] == b["num_scans"] and a["step"] == b["step"]
            np.testing.assert_array_equal(a["bounds"], b["bounds"], err_msg=f"source {k}")
            np.testing.assert_array_equal(a["sums"], b["sums"], err_msg=f"source {k}")
            np.testing.assert_array_equal(a["scans"], b["scans"], err_msg=f"source {k}")


# ---- b. every depth ----------------------------------------------------------------------------
@pytest.mark.parametrize("depth", range(1, 8))
def test_depths(sm, scene, built, depth):
    """Depth 1 has no quad layouts, depth 2 no planes for the 120 x 120 grid, depth 7 the most
    launches."""
    grids = [built.grids[0], built.grids[2], built.grids[1]]
    batch = scene.batch(grids, depth)
    for k, grid in enumerate(grids):
        _assert_same_levels(batch[k], scene.single(grid, depth), depth, f"source {k}")
    # the small grids searched once each (quads, planes and group planes in use)
    cloud = scene.clouds[2]
    for k, grid in enumerate(grids):
        one = scene.single(grid, depth)
        initial = scene.initial[2] if k == 1 else sm.Rigid2d(0.3, 0.3, 0.1)
        _assert_same_result(batch[k].match(initial, cloud, 0.05),
                            one.match(initial, cloud, 0.05), (depth, k))
        _assert_same_result(batch[k].match_full_submap(cloud, 0.05),
                            one.match_full_submap(cloud, 0.05), (depth, k, "full"))


# ---- c. use -------------------------------------------------------------------------------------
def test_searches_equal_the_single_creates(sm, scene, built):
    _assert_results_of_c(scene, built, built.batch, WITH_SCAN)


def test_match_pairs_over_batch_built_matchers(sm, scene, built):
    ks = [2, 3, 5, 2, 5, 3]
    full = [0, 1, 0, 1, 1, 0]
    initial = [scene.initial[k] for k in ks]
    clouds = [scene.clouds[k] for k in ks]
    min_scores = [built.thresholds[k][p % 2] for p, k in enumerate(ks)]
    got = sm.match_pairs([built.batch[k] for k in ks], initial, full, min_scores, clouds)
    want = sm.match_pairs([built.singles[k] for k in ks], initial, full, min_scores, clouds)
    np.testing.assert_array_equal(got[0], want[0])
    assert 0 < int(got[0].sum()) < len(ks)
    for p in range(len(ks)):
        _assert_same_result((bool(got[0][p]), got[1][p], got[2][p]),
                            (bool(want[0][p]), want[1][p], want[2][p]), p)
    for name in ("num_scans", "coarse_candidates"):
        assert got[3][name] == want[3][name]


def test_refinement_reads_the_batch_built_copy_of_the_cells(sm, scene, built):
    ceres = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, True, 10)
    steps = 0
    for k in WITH_SCAN:
        a = ceres.refine_batch([built.batch[k]], [1], [scene.initial[k]], scene.clouds[k])
        b = ceres.refine_batch([built.singles[k]], [1], [scene.initial[k]], scene.clouds[k])
        assert _xyt(a[0][0]) == _xyt(b[0][0]) and a[1] == b[1], k
        steps += a[1][0]["num_successful_steps"]
    assert steps > 0
    # all of them in one launch
    ks = list(WITH_SCAN)
    ceres_pairs = ceres.refine_pairs([built.batch[k] for k in ks], None,
                                     [scene.initial[k] for k in ks],
                                     [scene.clouds[k] for k in ks])
    want = ceres.refine_pairs([built.singles[k] for k in ks], None,
                              [scene.initial[k] for k in ks], [scene.clouds[k] for k in ks])
    assert [_xyt(p) for p in ceres_pairs[0]] == [_xyt(p) for p in want[0]]
    assert ceres_pairs[1] == want[1]


# ---- d. lifetime --------------------------------------------------------------------------------
def test_matchers_outlive_sources_and_batch_mates(sm, scene, built):
    grids = scene.sources()
    batch = scene.batch(grids, DEPTH)
    grids[1].__del__()                              # the resident TSDF, right after the call
    # the resident probability grid survives and changes; so do the host cells
    pose = scene.world_big.free_pose(77, 0.4)
    grids[3].insert(pose[:2], _in_map(pose, scene.world_big.scan(pose, 300, 10.0, 0.01, 7)))
    for k in (0, 2, 4, 5):
        grids[k].cells[...] = 0
    batch[0].__del__()                              # two of the batch, not the last ones
    batch[2].__del__()
    # device memory handed out again must not be the survivors'
    scratch = [scene.single(built.grids[2], DEPTH) for _ in range(3)]
    _assert_results_of_c(scene, built, batch, (3, 5))
    for k in (1, 3, 4, 5):
        _assert_same_levels(batch[k], built.singles[k], DEPTH, f"source {k}")
    grids[3].__del__()
    del scratch
    _assert_results_of_c(scene, built, batch, (3, 5))
    ceres = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, True, 10)
    assert ceres.refine_batch([batch[3]], [1], [scene.initial[3]], scene.clouds[3]) == \
        ceres.refine_batch([built.singles[3]], [1], [scene.initial[3]], scene.clouds[3])
    for k in (5, 1, 4, 3):                          # any order
        batch[k].__del__()


# ---- e. splitting -------------------------------------------------------------------------------
def test_chains_of_two(sm, scene, built, debug):
    """fast2d_create_chain = 2: the six sources go out as three chains of launches."""
    debug(fast2d_create_chain=2)
    batch = scene.batch(built.grids, DEPTH)
    for k in range(6):
        _assert_same_levels(batch[k], built.singles[k], DEPTH, f"source {k}")
    _assert_results_of_c(scene, built, batch, WITH_SCAN)
    debug(fast2d_create_chain=1)                    # and one by one
    batch = scene.batch(built.grids[:3], DEPTH)
    for k in range(3):
        _assert_same_levels(batch[k], built.singles[k], DEPTH, f"source {k}")


# ---- errors on the device path ------------------------------------------------------------------
def test_a_bad_source_builds_nothing(sm, scene, built):
    from cartographer_amd import _lib
    bad = sm.Grid2D(np.zeros((4, 4), np.uint16), RES, 0.2, 0.2, -1.5, 1.5)
    with pytest.raises(_lib.CmxError, match="source 2") as info:
        scene.batch([built.grids[0], built.grids[3], bad], DEPTH)
    assert info.value.status == _lib.INVALID_ARGUMENT
    with pytest.raises(_lib.CmxError, match="source 1") as info:
        sm.FastCorrelativeScanMatcher2D.create_batch([built.grids[0], built.grids[3]], DEPTH,
                                                     LIN, ANG, device=1 << 20)
    assert info.value.status == _lib.INVALID_ARGUMENT
    # nothing launched afterwards fails
    _assert_results_of_c(scene, built, built.batch, (2,))


# ---- f. ConstraintBuilder2D(batch_create=True) ------------------------------------------------
@pytest.mark.parametrize("pairs", [False, True])
def test_builder_with_and_without_batch_create(sm, synth, pairs):
    """Four nodes against three submaps, windowed and global pairs: the same constraint list
    whether the matchers are built one by one or in one call at the flush."""
    from cartographer_amd import constraint_builder as cb
    options = cb.ConstraintBuilderOptions(
        sampling_ratio=1.0, min_score=0.4, global_localization_min_score=0.45,
        linear_search_window=LIN, angular_search_window=ANG, branch_and_bound_depth=5)
    submaps, world = [], None
    for seed, nx, ny in ((11, 120, 120), (12, 96, 150), (13, 150, 96)):
        cells, lim, w = synth.make_submap(seed, nx, ny, RES, 12, 400, 5.0, 0.01)
        world = world or w
        submaps.append(cb.Submap2D(sm.Rigid2d(0.0, 0.0, 0.0),
                                   sm.Grid2D(cells, RES, lim["max_x"], lim["max_y"])))
    nodes = []
    for k in range(4):
        truth = world.free_pose(80 + k, 0.3)
        nodes.append((truth, world.scan(truth, 250 - 30 * k, 5.0, 0.01, k)))
    lists = []
    for batch_create in (False, True):
        builder = cb.ConstraintBuilder2D(options, pairs=pairs, batch_create=batch_create)
        for k, (truth, cloud) in enumerate(nodes):
            relative = sm.Rigid2d(float(truth[0] + 0.1), float(truth[1] - 0.05),
                                  float(truth[2] + 0.02))
            for j in range(2 if k else 3):          # the third submap joins through node 0 ...
                builder.maybe_add_constraint((0, j), submaps[j], (0, k), cloud, relative)
            if k % 2 == 0:
                builder.maybe_add_global_constraint((0, 0), submaps[0], (0, k), cloud)
            if k == 3:                              # ... and a global pair of the last node
                builder.maybe_add_global_constraint((0, 2), submaps[2], (0, k), cloud)
            assert builder.num_scan_matchers() == 3
            if k == 1:
                builder.notify_end_of_node()        # a flush in the middle: later ones build nothing
        out = []
        builder.when_done(out.extend)
        lists.append(out)
    assert len(lists[0]) >= 3 and lists[0] == lists[1]
    assert any(c.submap_id == (0, 0) for c in lists[0])
