"""cmx_fast2d_match_pairs / cmx_fast2d_refine_pairs / cmx_ceres2d_refine_pairs_tsdf: many nodes
against 2D submaps in one call (the burst of PoseGraph2D::ComputeConstraintsForNode when a submap
finishes, pose_graph_2d.cc:383-393), and matchers built from resident grids without a host copy.

Expected values are always the single calls' results (cmx_fast2d_match, match_full_submap,
refine_batch, refine_batch_tsdf of one pair), which the rest of the suite pins to the oracle:
found flag equal, f32 score bit-equal, pose at atol = 0, summaries field by field.

Of cmx_match_stats only num_scans and coarse_candidates are compared: they are functions of the
inputs.  The work counters of the tree search (candidates_scored, nodes_expanded, expansion_*)
depend on when the bound rises and differ between two runs of the same call.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES = 0.05
LIN, ANG = 1.0, math.radians(20.0)
OFFSETS = [(0.1, -0.05, 0.02), (-0.15, 0.1, -0.03), (0.05, 0.2, 0.04)]
CUTS = [384, 257, 256, 129, 65, 64, 63, 2, 1]     # wave / block boundaries, the smallest clouds


@pytest.fixture(scope="module")
def sm():
    from cartographer_amd import _lib, scan_matching
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching


def _grid(sm, cells, lim):
    return sm.Grid2D(cells, RES, lim["max_x"], lim["max_y"])


def _submap(synth, seed, nx, ny):
    return synth.make_submap(seed, nx, ny, RES, 12, 400, 5.0, 0.01)


def _xyt(pose):
    return [pose.x, pose.y, pose.theta]


def _single(sm, matcher, initial, full, min_score, cloud):
    """(found, score, pose, stats) of the single call for one pair."""
    got = (matcher.match_full_submap(cloud, min_score) if full else
           matcher.match(initial, cloud, min_score))
    return got + (dict(matcher.last_stats),)


def _assert_pairs_equal_singles(got, singles):
    found, scores, poses, _ = got
    for k, one in enumerate(singles):
        assert bool(found[k]) == bool(one[0]), f"pair {k}"
        if not one[0]:
            continue
        assert np.float32(scores[k]) == np.float32(one[1]), f"pair {k}"
        np.testing.assert_allclose(_xyt(poses[k]), _xyt(one[2]), rtol=0, atol=0,
                                   err_msg=f"pair {k}")


def _assert_same_results(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1][a[0] != 0], b[1][b[0] != 0])
    for k in np.nonzero(a[0])[0]:
        assert _xyt(a[2][k]) == _xyt(b[2][k]), f"pair {k}"


# ----------------------------------------------------------------------------
# Scene 1: old nodes against one submap
# ----------------------------------------------------------------------------
class OldNodes:
    """One depth-5 matcher, nine nodes with scans from different free poses, cut to CUTS points;
    windowed around offset initial poses.  The threshold lies between the fifth and the sixth
    best of the nine scores, so that found and not-found pairs both occur."""

    def __init__(self, sm, synth):
        cells, lim, world = _submap(synth, 11, 120, 120)
        self.matcher = sm.FastCorrelativeScanMatcher2D(_grid(sm, cells, lim), 5, LIN, ANG)
        self.clouds, self.initial = [], []
        for k, cut in enumerate(CUTS):
            truth = world.free_pose(20 + k, 0.3)
            scan = world.scan(truth, 500, 5.0, 0.01, k)
            assert len(scan) >= cut
            self.clouds.append(np.ascontiguousarray(scan[:cut]))
            self.initial.append(sm.Rigid2d(*[float(t + o) for t, o in
                                             zip(truth, OFFSETS[k % 3])]))
        num = len(CUTS)
        scores = [self.matcher.match(self.initial[k], self.clouds[k], 0.0)[1] for k in range(num)]
        assert all(s is not None for s in scores)
        ranked = sorted(scores)
        self.min_score = float(np.float32(0.5 * (ranked[3] + ranked[4])))
        assert ranked[3] < self.min_score < ranked[4]
        self.singles = [_single(sm, self.matcher, self.initial[k], False, self.min_score,
                                self.clouds[k]) for k in range(num)]
        self.matchers = [self.matcher] * num

    def pairs(self, sm, clouds=None):
        num = len(CUTS)
        return sm.match_pairs(self.matchers, self.initial, [0] * num, [self.min_score] * num,
                              self.clouds if clouds is None else clouds)


@pytest.fixture(scope="module")
def old_nodes(sm, synth):
    return OldNodes(sm, synth)


def test_old_nodes_against_one_submap(sm, old_nodes):
    got = old_nodes.pairs(sm)
    _assert_pairs_equal_singles(got, old_nodes.singles)
    assert 0 < int(got[0].sum()) < len(CUTS)            # found and not-found pairs both occur
    assert got[3]["num_scans"] == sum(s[3]["num_scans"] for s in old_nodes.singles)
    assert got[3]["coarse_candidates"] == sum(s[3]["coarse_candidates"]
                                              for s in old_nodes.singles)


def test_resident_clouds_equal_host_arrays(sm, old_nodes):
    resident = [sm.PointCloudOnDevice(c) for c in old_nodes.clouds]
    _assert_same_results(old_nodes.pairs(sm, resident), old_nodes.pairs(sm))
    _assert_pairs_equal_singles(old_nodes.pairs(sm, resident), old_nodes.singles)


# ----------------------------------------------------------------------------
# Scene 2: cross product with repeats
# ----------------------------------------------------------------------------
class Cross:
    """Three nodes x four matchers of depths 3, 4, 6 and 4 on grids of unlike sizes; windowed and
    full-submap pairs mixed, thresholds of their own; every pair of a node names the node's one
    cloud object."""

    def __init__(self, sm, synth):
        shapes = [(12, 96, 150, 3), (11, 120, 120, 4), (11, 120, 120, 6), (13, 150, 96, 4)]
        self.bank = []
        world = None                       # the nodes' scans are taken in the world of seed 11
        for seed, nx, ny, depth in shapes:
            cells, lim, w = _submap(synth, seed, nx, ny)
            world = w if seed == 11 and world is None else world
            self.bank.append(sm.FastCorrelativeScanMatcher2D(_grid(sm, cells, lim), depth, LIN,
                                                             ANG))
        self.node_clouds, truths = [], []
        for i, beams in enumerate((300, 200, 150)):
            truth = world.free_pose(40 + i, 0.3)
            truths.append(truth)
            self.node_clouds.append(world.scan(truth, beams, 5.0, 0.01, 7 + i))
        self.matchers, self.clouds, self.initial, self.full, self.min_scores = [], [], [], [], []
        for i in range(3):
            for j in range(4):
                self.matchers.append(self.bank[j])
                self.clouds.append(self.node_clouds[i])          # the same object for the node
                self.initial.append(sm.Rigid2d(*[float(t + o) for t, o in
                                                 zip(truths[i], OFFSETS[(i + j) % 3])]))
                self.full.append(1 if (i + j) % 3 == 0 else 0)
                self.min_scores.append(0.15 + 0.05 * ((4 * i + j) % 4))
        self.num = len(self.matchers)
        self.singles = [_single(sm, self.matchers[p], self.initial[p], self.full[p],
                                self.min_scores[p], self.clouds[p]) for p in range(self.num)]

    def pairs(self, sm, order=None, clouds=None):
        order = range(self.num) if order is None else order
        clouds = self.clouds if clouds is None else clouds
        return sm.match_pairs([self.matchers[p] for p in order], [self.initial[p] for p in order],
                              [self.full[p] for p in order], [self.min_scores[p] for p in order],
                              [clouds[p] for p in order])


@pytest.fixture(scope="module")
def cross(sm, synth):
    return Cross(sm, synth)


def test_cross_product_with_repeats(sm, cross):
    assert {m.options.branch_and_bound_depth for m in cross.matchers} == {3, 4, 6}
    assert 0 < sum(cross.full) < cross.num
    got = cross.pairs(sm)
    _assert_pairs_equal_singles(got, cross.singles)
    assert got[0].any()
    assert got[3]["num_scans"] == sum(s[3]["num_scans"] for s in cross.singles)
    assert got[3]["coarse_candidates"] == sum(s[3]["coarse_candidates"] for s in cross.singles)
    order = list(np.random.default_rng(3).permutation(cross.num))
    shuffled = cross.pairs(sm, order)
    _assert_pairs_equal_singles(shuffled, [cross.singles[p] for p in order])
    assert shuffled[3]["num_scans"] == got[3]["num_scans"]


def test_one_group_is_the_old_batch(sm, cross):
    """Pairs that all share one cloud (and one depth): what cmx_fast2d_match_batch returns."""
    picks = [1, 3, 1, 3]        # node 0 against the depth-4 matchers (its own world, another)
    initial = [cross.initial[p] for p in picks]
    full, thresholds = [0, 1, 1, 0], [0.2, 0.3, 0.25, 0.95]
    matchers = [cross.matchers[p] for p in picks]
    cloud = cross.node_clouds[0]
    batch = sm.match_batch(matchers, initial, full, thresholds, cloud)
    got = sm.match_pairs(matchers, initial, full, thresholds, [cloud] * len(picks))
    np.testing.assert_array_equal(got[0], batch[0])
    np.testing.assert_array_equal(got[1], batch[1])
    assert [_xyt(p) for p in got[2]] == [_xyt(p) for p in batch[2]]
    for key in ("num_scans", "coarse_candidates"):
        assert got[3][key] == batch[3][key], key
    assert got[0].any() and not got[0].all()


def test_stream_override(sm, cross):
    """Under cmx_set_stream the groups run one after the other on the caller's stream."""
    import torch
    from cartographer_amd import _lib
    stream = torch.cuda.Stream()
    _lib.check(_lib.lib().cmx_set_stream(0, C.c_void_p(stream.cuda_stream)))
    try:
        got = cross.pairs(sm)
        stream.synchronize()
    finally:
        _lib.check(_lib.lib().cmx_set_stream(0, None))
    _assert_pairs_equal_singles(got, cross.singles)
    assert got[3]["num_scans"] == sum(s[3]["num_scans"] for s in cross.singles)


# ----------------------------------------------------------------------------
# Refinement
# ----------------------------------------------------------------------------
def _assert_refined_pair_by_pair(ceres, got, matchers, found, poses, clouds):
    refined, summaries = got
    for p in range(len(matchers)):
        flag = 1 if found is None else int(found[p])
        one, summary = ceres.refine_batch([matchers[p]], [flag], [poses[p]], clouds[p])
        assert _xyt(refined[p]) == _xyt(one[0]), f"pair {p}"
        assert summaries[p] == summary[0], f"pair {p}"
        if not flag:
            assert _xyt(refined[p]) == _xyt(poses[p])      # passed through


@pytest.mark.parametrize("scene", ["old_nodes", "cross"])
def test_refine_pairs_equals_refine_batch_pair_by_pair(sm, request, scene):
    s = request.getfixturevalue(scene)
    ceres = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, True, 10)
    found, _, poses, _ = s.pairs(sm)
    assert found.any() and (scene != "old_nodes" or not found.all())
    got = ceres.refine_pairs(s.matchers, found, poses, s.clouds)
    _assert_refined_pair_by_pair(ceres, got, s.matchers, found, poses, s.clouds)
    assert any(summary["num_successful_steps"] > 0 for summary in got[1])
    # found = None: every pair is refined, from whatever pose it has
    everything = ceres.refine_pairs(s.matchers, None, poses, s.clouds)
    _assert_refined_pair_by_pair(ceres, everything, s.matchers, None, poses, s.clouds)
    # resident clouds: the same, and one object per node stays one object
    resident_of = {id(c): sm.PointCloudOnDevice(c) for c in s.clouds}
    resident = [resident_of[id(c)] for c in s.clouds]
    again = ceres.refine_pairs(s.matchers, found, poses, resident)
    assert [_xyt(p) for p in again[0]] == [_xyt(p) for p in got[0]]
    assert again[1] == got[1]


def test_refine_pairs_on_tsdf(sm, synth, oracle):
    """Three resident TSDF2D grids, five clouds of unlike sizes, one of them empty."""
    import tsdf_helpers
    from cartographer_amd import grid_2d
    T, W = 0.3, 10.0
    grids, world = [], None
    for seed, nx, ny in ((11, 120, 120), (12, 96, 150), (13, 110, 100)):
        cells, lim, w = _submap(synth, seed, nx, ny)
        world = world or w
        tsd, wgt = tsdf_helpers.tsdf_from_probability_grid(oracle, cells, RES, T, W, seed)
        grids.append(grid_2d.TSDF2DOnDevice(RES, (lim["max_x"], lim["max_y"]), nx, ny, T, W, tsd,
                                            wgt))
    truth = world.free_pose(61, 0.3)
    scan = world.scan(truth, 400, 5.0, 0.01, 3)
    assert len(scan) >= 300
    # (arrays of their own: slices of one array would be one pointer with unlike num_points)
    clouds = [scan[:n].copy() for n in (300, 129, 64, 1)] + [np.zeros((0, 3), np.float32)]
    picks = [(0, 0), (1, 1), (2, 2), (0, 3), (1, 4), (0, 1), (2, 0)]      # (grid, cloud)
    pair_grids = [grids[g] for g, _ in picks]
    pair_clouds = [clouds[c] for _, c in picks]
    poses = [sm.Rigid2d(*[float(t + o) for t, o in zip(truth, OFFSETS[k % 3])])
             for k in range(len(picks))]
    found = np.array([1, 1, 1, 1, 1, 0, 1], np.int32)
    ceres = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, True, 10)
    for flags in (found, None):
        refined, summaries = ceres.refine_pairs_tsdf(pair_grids, flags, poses, pair_clouds)
        for p in range(len(picks)):
            flag = None if flags is None else [int(flags[p])]
            one, summary = ceres.refine_batch_tsdf([pair_grids[p]], flag, [poses[p]],
                                                   pair_clouds[p])
            assert _xyt(refined[p]) == _xyt(one[0]), f"pair {p}"
            assert summaries[p] == summary[0], f"pair {p}"
        # the empty cloud: FAILURE, the pose untouched
        assert summaries[4]["termination"] == 2 and _xyt(refined[4]) == _xyt(poses[4])
        assert summaries[0]["termination"] != 2
        assert any(summary["num_successful_steps"] > 0 for summary in summaries)


# ----------------------------------------------------------------------------
# Argument errors
# ----------------------------------------------------------------------------
def _raw_match_pairs(matchers, pointers, counts, num_pairs, full, with_initial=True):
    """cmx_fast2d_match_pairs through ctypes: (status, error text)."""
    from cartographer_amd import _lib
    L = _lib.lib()
    num = len(pointers)
    handles = (C.c_void_p * num)(*[m._h if m is not None else None for m in matchers])
    initial = (_lib.Pose2d * num)()
    flags = (C.c_int32 * num)(*full)
    thresholds = (C.c_float * num)(*([0.2] * num))
    found, scores = (C.c_int32 * num)(), (C.c_float * num)()
    poses = (_lib.Pose2d * num)()
    status = L.cmx_fast2d_match_pairs(
        handles, num_pairs, C.cast(initial, C.c_void_p) if with_initial else None,
        C.cast(flags, C.c_void_p), C.cast(thresholds, C.c_void_p),
        (C.c_void_p * num)(*pointers), C.cast((C.c_int32 * num)(*counts), C.c_void_p),
        C.cast(found, C.c_void_p), C.cast(scores, C.c_void_p), C.cast(poses, C.c_void_p), None)
    return status, L.cmx_last_error().decode()


def test_argument_errors(sm, cross):
    from cartographer_amd import _lib
    cloud, other = cross.node_clouds[0], cross.node_clouds[1]
    a, b = cloud.ctypes.data, other.ctypes.data
    two = [cross.bank[1], cross.bank[3]]
    cases = [
        # equal cloud pointers with different num_points
        (two, [a, a], [len(cloud), len(cloud) - 1], 2, [0, 0], True, "num_points"),
        # a windowed pair without initial poses
        (two, [a, b], [len(cloud), len(other)], 2, [1, 0], False, "initial_pose_estimates"),
        # no pairs
        (two, [a, b], [len(cloud), len(other)], 0, [0, 0], True, "num_pairs"),
        # a null matcher
        ([cross.bank[1], None], [a, b], [len(cloud), len(other)], 2, [0, 0], True, "null matcher"),
        # a null and an empty cloud
        (two, [a, None], [len(cloud), len(other)], 2, [0, 0], True, "null"),
        (two, [a, b], [len(cloud), 0], 2, [0, 0], True, "empty point cloud"),
    ]
    for matchers, pointers, counts, num_pairs, full, with_initial, word in cases:
        status, error = _raw_match_pairs(matchers, pointers, counts, num_pairs, full, with_initial)
        assert status == _lib.INVALID_ARGUMENT and word in error, (word, status, error)
        # nothing launched afterwards fails
        _assert_pairs_equal_singles(
            sm.match_pairs([cross.matchers[1]], [cross.initial[1]], [cross.full[1]],
                           [cross.min_scores[1]], [cross.clouds[1]]), [cross.singles[1]])
    # every pair a full-submap search: no initial poses needed
    status, error = _raw_match_pairs(two, [a, b], [len(cloud), len(other)], 2, [1, 1], False)
    assert status == _lib.OK, error
    # the refinement refuses the same lists
    ceres = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, True, 10)
    with pytest.raises(_lib.CmxError, match="num_points") as info:
        ceres.refine_pairs(two, None, [sm.Rigid2d()] * 2, [cloud, cloud[:-1]])
    assert info.value.status == _lib.INVALID_ARGUMENT
    with pytest.raises(_lib.CmxError, match="num_pairs") as info:
        ceres.refine_pairs([], None, [], [])
    assert info.value.status == _lib.INVALID_ARGUMENT


# ----------------------------------------------------------------------------
# ConstraintBuilder2D(pairs=True)
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("with_ceres", [False, True])
def test_builder_with_and_without_pairs(sm, synth, with_ceres):
    """A burst of six nodes against two submaps: the same constraint list either way."""
    from cartographer_amd import constraint_builder as cb
    options = cb.ConstraintBuilderOptions(
        sampling_ratio=1.0, min_score=0.4, global_localization_min_score=0.45,
        linear_search_window=LIN, angular_search_window=ANG, branch_and_bound_depth=5)
    submaps, world = [], None
    for seed, nx, ny in ((11, 120, 120), (12, 96, 150)):
        cells, lim, w = _submap(synth, seed, nx, ny)
        world = world or w
        submaps.append(cb.Submap2D(sm.Rigid2d(0.0, 0.0, 0.0), _grid(sm, cells, lim)))
    nodes = []
    for k in range(6):
        truth = world.free_pose(80 + k, 0.3)
        nodes.append((truth, world.scan(truth, 250 - 30 * k, 5.0, 0.01, k)))
    lists = []
    for pairs in (False, True):
        ceres = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, True, 10) if with_ceres else None
        builder = cb.ConstraintBuilder2D(options, ceres=ceres, pairs=pairs)
        for k, (truth, cloud) in enumerate(nodes):
            relative = sm.Rigid2d(*[float(t + o) for t, o in zip(truth, OFFSETS[k % 3])])
            for j, submap in enumerate(submaps):
                builder.maybe_add_constraint((0, j), submap, (0, k), cloud, relative)
            if k % 2 == 0:
                builder.maybe_add_global_constraint((0, 0), submaps[0], (0, k), cloud)
        out = []
        builder.when_done(out.extend)
        lists.append(out)
    assert len(lists[0]) >= 3 and lists[0] == lists[1]


# ----------------------------------------------------------------------------
# Matchers built from resident grids
# ----------------------------------------------------------------------------
def _in_map(pose, points):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    out = np.array(points, np.float32, copy=True)
    out[:, 0] = pose[0] + c * points[:, 0] - s * points[:, 1]
    out[:, 1] = pose[1] + s * points[:, 0] + c * points[:, 1]
    return out


@pytest.mark.parametrize("kind", ["probability", "tsdf"])
def test_matcher_from_a_resident_grid(sm, synth, oracle, kind):
    """Every level of from_device_grid equals the matcher built from the downloaded cells; the
    grid is destroyed before the matches: the matcher holds its own copy."""
    from cartographer_amd import grid_2d
    cells, lim, world = _submap(synth, 11, 120, 120)
    truth = world.free_pose(5, 0.4)
    scan = world.scan(truth, 300, 5.0, 0.01, 9)
    if kind == "probability":
        device_grid = grid_2d.ProbabilityGridOnDevice(RES, (lim["max_x"] + 1.0, lim["max_y"] + 0.5),
                                                      160, 150)
        for k in range(4):
            pose = world.free_pose(30 + k, 0.4)
            device_grid.insert(pose[:2], _in_map(pose, world.scan(pose, 300, 5.0, 0.01, k)))
        device_grid.crop()
        now = device_grid.limits
        assert (now["num_x_cells"], now["num_y_cells"]) != (160, 150)
        host = sm.Grid2D(device_grid.cells, RES, now["max_x"], now["max_y"])
    else:
        import tsdf_helpers
        tsd, wgt = tsdf_helpers.tsdf_from_probability_grid(oracle, cells, RES, 0.3, 10.0, 4)
        device_grid = grid_2d.TSDF2DOnDevice(RES, (lim["max_x"], lim["max_y"]), 120, 120, 0.3,
                                             10.0, tsd, wgt)
        host = sm.Grid2D(device_grid.planes()[0], RES, lim["max_x"], lim["max_y"], -0.3, 0.3)
    for depth in range(1, 7):
        resident = sm.FastCorrelativeScanMatcher2D.from_device_grid(device_grid, depth, LIN, ANG)
        uploaded = sm.FastCorrelativeScanMatcher2D(host, depth, LIN, ANG)
        for level in range(depth):
            np.testing.assert_array_equal(resident.level(level), uploaded.level(level))
    device_grid.__del__()                                  # the depth-6 matchers outlive the grid
    initial = sm.Rigid2d(truth[0] + 0.1, truth[1] - 0.05, truth[2] + 0.02)
    for min_score in (0.05, 0.3):
        a = resident.match_full_submap(scan, min_score)
        b = uploaded.match_full_submap(scan, min_score)
        assert a[0] == b[0] and a[1] == b[1] and (not a[0] or _xyt(a[2]) == _xyt(b[2]))
        a = resident.match(initial, scan, min_score)
        b = uploaded.match(initial, scan, min_score)
        assert a[0] == b[0] and a[1] == b[1] and (not a[0] or _xyt(a[2]) == _xyt(b[2]))
    # the refinement reads the matcher's copy of the cells too
    ceres = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, True, 10)
    if kind == "probability":
        assert ceres.refine_batch([resident], [1], [initial], scan) == \
            ceres.refine_batch([uploaded], [1], [initial], scan)
