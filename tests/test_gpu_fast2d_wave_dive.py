"""The dive of the fast 2D matcher by one wavefront per seed (fast_2d_seed.hip, DiveWaveKernel; debug
switch fast2d_dive = 2) against the dive by one workgroup per seed (DiveKernel, fast2d_dive = 1) and
against the oracle, and the fused front end (fast_2d_coarse.hip, PrepScoreFusedKernel) against the
oracle's cells, bounds and sums.  Bars as in test_gpu_queue.py: found flag and f32 score bit-equal,
pose to 1e-12 (f64 from integer offsets).

Between the two dives `coarse_candidates` and `num_scans` are compared in every case.
`candidates_scored` is the dives' share (the same seeds, the same walks: equal) plus the tree
search's, and the tree search's depends on when its wavefronts see the bound rise
(test_gpu_queue.py::test_queue_search_counts_its_work, test_gpu_r2_paths.py).  It is compared, with
`nodes_expanded`, wherever the tree's share does not depend on timing, which is wherever the bound
cannot move once the dives have run:
  * depth 1 (no dive, no tree);
  * a windowed search of a grid of equal cells: every candidate has the dive's score, the bound
    is final from the first dive on and the tree expands every node (grouped and not, 1 and 300
    points -- the gathers of four and of eight cells a lane --, children beyond the bounds);
  * a threshold no candidate reaches: no seed, nothing passes the filter;
  * bench.py's scan #0 under exact lowest-resolution scores, whose dive finds the optimum.
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIVES = (2, 1)      # the wave dive wherever it is possible, the block dive


@pytest.fixture(scope="module")
def sm():
    from cartographer_amd import _lib, scan_matching
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching


@pytest.fixture(scope="module")
def small(synth):
    """A 100 x 100 grid and a scan of 1100 points of it (cases take the first n)."""
    cells, lim, world = synth.make_submap(11, 100, 100, 0.05, 8, 400, 30.0, 0.01)
    scan = world.scan(world.free_pose(5, 0.5), 1100, 30.0, 0.01, 2)
    assert scan.shape[0] == 1100
    return cells, lim, world, scan


@pytest.fixture(scope="module")
def odd(synth):
    """37 x 53: divides nothing."""
    cells, lim, world = synth.make_submap(13, 37, 53, 0.05, 4, 200, 30.0, 0.01)
    scan = world.scan(world.free_pose(3, 0.3), 300, 30.0, 0.01, 4)
    return cells, lim, world, scan


@pytest.fixture(scope="module")
def big(synth):
    """bench.py's C2 world (400 x 400, depth 7) and the first two scans of its headline."""
    cells, lim, world = synth.make_submap(42, 400, 400, 0.05, 30, 1000, 30.0, 0.01)
    scans = [world.scan(world.free_pose(1234 + k, 0.5), 1000, 30.0, 0.01, 7 + k) for k in range(2)]
    return cells, lim, world, scans


def _matcher(sm, cells, lim, depth, **kw):
    return sm.FastCorrelativeScanMatcher2D(
        sm.Grid2D(cells, lim["resolution"], lim["max_x"], lim["max_y"]), depth, **kw)


def _oracle(oracle, cells, lim, depth, *window):
    return oracle.FastCorrelativeScanMatcher2D(cells, lim["resolution"], lim["max_x"], lim["max_y"],
                                               depth, *window)


def _xyt(pose):
    return (pose.x, pose.y, pose.theta) if hasattr(pose, "theta") else tuple(np.asarray(pose)[:3])


def _same(got, ref):
    found, score, pose = got
    assert bool(found) == bool(ref["found"])
    if ref["found"]:
        assert np.float32(score) == np.float32(ref["score"])
        assert np.max(np.abs(np.asarray(_xyt(pose)) - np.asarray(ref["pose"][:3]))) < 1e-12


def _both_dives(debug, gm, run, ref, scored_too=False, **switches):
    """run() under either dive: equal to the oracle's `ref`; the statistics of the two compared."""
    stats = []
    for dive in DIVES:
        debug(fast2d_dive=dive, **switches)
        _same(run(), ref)
        stats.append(dict(gm.last_stats))
    wave, block = stats
    print("candidates_scored wave / block:", wave["candidates_scored"], block["candidates_scored"])
    print("nodes_expanded wave / block:", wave["nodes_expanded"], block["nodes_expanded"])
    for key in ("coarse_candidates", "num_scans") + (
            ("candidates_scored", "nodes_expanded") if scored_too else ()):
        assert wave[key] == block[key], key
    return wave


# 1024: the last size a wavefront holds; 1025: routed to the block dive under either switch
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 1024, 1025])
@pytest.mark.parametrize("depth", [4, 5])
def test_wave_dive_point_counts(sm, oracle, small, debug, n, depth):
    cells, lim, _, scan = small
    cloud = np.ascontiguousarray(scan[:n])
    ref = _oracle(oracle, cells, lim, depth).match_full_submap(cloud, 0.3)
    gm = _matcher(sm, cells, lim, depth)
    _both_dives(debug, gm, lambda: gm.match_full_submap(cloud, 0.3), ref)


@pytest.mark.parametrize("depth", [1, 2, 4, 5, 7])
def test_wave_dive_depths(sm, oracle, small, debug, depth):
    """Depth 1 launches no dive (the result and every count unchanged); 5 is the first depth under
    group bounds."""
    cells, lim, _, scan = small
    cloud = np.ascontiguousarray(scan[:300])
    ref = _oracle(oracle, cells, lim, depth).match_full_submap(cloud, 0.4)
    gm = _matcher(sm, cells, lim, depth)
    _both_dives(debug, gm, lambda: gm.match_full_submap(cloud, 0.4), ref, scored_too=depth == 1)


@pytest.mark.parametrize("depth", [2, 5])
def test_wave_dive_on_a_grid_that_divides_nothing(sm, oracle, odd, debug, depth):
    cells, lim, _, scan = odd
    ref = _oracle(oracle, cells, lim, depth).match_full_submap(scan, 0.3)
    gm = _matcher(sm, cells, lim, depth)
    _both_dives(debug, gm, lambda: gm.match_full_submap(scan, 0.3), ref)


def test_wave_dive_on_the_bench_world(sm, oracle, big, debug):
    """400 x 400 at depth 7, as shipped (group bounds) and with exact lowest-resolution scores,
    where the dive of scan #0 finds the optimum: every path then expands exactly the nodes that
    reach the final bound, and the work counters of the two dives are equal."""
    cells, lim, _, scans = big
    om = _oracle(oracle, cells, lim, 7)
    gm = _matcher(sm, cells, lim, 7)
    refs = [om.match_full_submap(s, 0.6) for s in scans]
    for scan, ref in zip(scans, refs):
        assert ref["found"]
        _both_dives(debug, gm, lambda: gm.match_full_submap(scan, 0.6), ref)
    exact = _both_dives(debug, gm, lambda: gm.match_full_submap(scans[0], 0.6), refs[0],
                        scored_too=True, fast2d_group=1)
    assert exact["nodes_expanded"] == 3076


@pytest.mark.parametrize("depth", [4, 5, 7])
def test_wave_dive_window_smaller_than_a_lowest_resolution_cell(sm, oracle, small, debug, depth):
    """A window of two cells either way against lowest-resolution cells of 8 - 64: one candidate
    per rotation, and below it children beyond the search bounds at every level."""
    cells, lim, world, scan = small
    cloud = np.ascontiguousarray(scan[:500])
    truth = world.free_pose(5, 0.5)
    init = [truth[0] + 0.05, truth[1] - 0.05, truth[2] + 0.02]
    window = (0.1, math.radians(10.0))
    ref = _oracle(oracle, cells, lim, depth, *window).match(init, cloud, 0.3)
    gm = _matcher(sm, cells, lim, depth, linear_search_window=window[0],
                  angular_search_window=window[1])
    _both_dives(debug, gm, lambda: gm.match(sm.Rigid2d(*init), cloud, 0.3), ref)


@pytest.mark.parametrize("switches", [
    {"fast2d_group": 1},                               # no group bounds: four seeds per workgroup
    {"fast2d_group": 2},                               # group bounds: a unit's three rotations
    {"fast2d_group": 2, "fast2d_group_verify": 1},     # ... every bound checked on the device
    {"fast2d_group": 2, "fast2d_group_verify": 2},     # ... every unit as if its premise had failed
], ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
@pytest.mark.parametrize("depth", [2, 5])
def test_wave_dive_with_and_without_group_bounds(sm, oracle, small, debug, depth, switches):
    cells, lim, world, scan = small
    cloud = np.ascontiguousarray(scan[:700])
    ref = _oracle(oracle, cells, lim, depth).match_full_submap(cloud, 0.4)
    gm = _matcher(sm, cells, lim, depth)
    _both_dives(debug, gm, lambda: gm.match_full_submap(cloud, 0.4), ref, **switches)
    truth = world.free_pose(5, 0.5)
    init = [truth[0] + 0.3, truth[1] - 0.2, truth[2] + 0.1]
    window = (2.0, math.radians(25.0))
    ref = _oracle(oracle, cells, lim, depth, *window).match(init, cloud, 0.3)
    gw = _matcher(sm, cells, lim, depth, linear_search_window=window[0],
                  angular_search_window=window[1])
    _both_dives(debug, gw, lambda: gw.match(sm.Rigid2d(*init), cloud, 0.3), ref, **switches)


@pytest.mark.parametrize("group", [1, 2], ids=["ungrouped", "grouped"])
@pytest.mark.parametrize("n", [1, 300])
def test_wave_dive_all_ties(sm, oracle, debug, n, group):
    """A grid of unknown cells: every candidate ties, the dive and the tree record the same leaf
    twice, and the leaf the reference's depth-first order meets first comes back
    (ConstraintBuilder2DTest's grid, as in test_gpu_queue.py).  The bound is final from the first
    dive on, so the work counters are the dives' share plus a constant: compared between the two
    dives, with three wavefronts a unit and four seeds a workgroup, four (n = 1) and eight
    (n = 300) cells a lane, and in the windowed search children beyond the bounds at every level
    (a window of 7 cells under lowest-resolution cells of 64)."""
    cells = np.zeros((110, 100), np.uint16)
    if n == 1:
        cloud = np.array([[0.1, 0.2, 0.3]], np.float32)
    else:
        cloud = np.zeros((n, 3), np.float32)
        cloud[:, :2] = np.random.default_rng(5).uniform(-3.0, 3.0, (n, 2)).astype(np.float32)
    om = oracle.FastCorrelativeScanMatcher2D(cells, 1.0, 2.0, 3.0, 7, 7.0, math.radians(30.0))
    gm = sm.FastCorrelativeScanMatcher2D(sm.Grid2D(cells, 1.0, 2.0, 3.0), 7,
                                         linear_search_window=7.0,
                                         angular_search_window=math.radians(30.0))
    ref_win = om.match([4.0, 5.0, 0.0], cloud, 0.0)
    _both_dives(debug, gm, lambda: gm.match(sm.Rigid2d(4.0, 5.0, 0.0), cloud, 0.0), ref_win,
                scored_too=True, fast2d_group=group)
    if n == 1:
        # (the full search expands 138 000 tied nodes, and that count was seen to differ by three
        # between two runs -- the tree's: a dive adds its six levels whatever it finds)
        ref_full = om.match_full_submap(cloud, 0.0)
        _both_dives(debug, gm, lambda: gm.match_full_submap(cloud, 0.0), ref_full,
                    fast2d_group=group)


@pytest.mark.parametrize("depth", [4, 5])
def test_wave_dive_with_few_or_no_seeds(sm, oracle, small, debug, depth):
    """A threshold just below the best score: a handful of rotations have a candidate above it,
    most seed numbers find nothing (the workgroups without a seed leave); and a threshold nothing
    reaches: no seed at all, found = 0 on both sides."""
    cells, lim, _, scan = small
    cloud = np.ascontiguousarray(scan[:700])
    om = _oracle(oracle, cells, lim, depth)
    gm = _matcher(sm, cells, lim, depth)
    best = om.match_full_submap(cloud, 0.3)
    assert best["found"]
    for threshold in (float(best["score"]) - 0.01, 0.99):
        ref = om.match_full_submap(cloud, threshold)
        _both_dives(debug, gm, lambda: gm.match_full_submap(cloud, threshold), ref,
                    scored_too=threshold == 0.99)
    assert not ref["found"]


@pytest.mark.parametrize("num", [3, 5])
def test_wave_dive_for_batches_of_unlike_submaps(sm, oracle, synth, small, odd, debug, num):
    """cmx_fast2d_match_batch over unlike submaps, full and windowed searches mixed: three
    problems go to the work queue, five to the level-synchronous launches."""
    cells, lim, world, scan = small
    cloud = np.ascontiguousarray(scan[:600])
    grids = [(cells, lim), odd[:2],
             synth.make_submap(17, 160, 120, 0.05, 10, 400, 30.0, 0.01)[:2]]
    window = (1.0, math.radians(20.0))
    truth = world.free_pose(5, 0.5)
    init = [truth[0] + 0.2, truth[1] - 0.1, truth[2] + 0.05]
    order = [0, 1, 2, 0, 2][:num]
    flags = [1, 1, 0, 0, 1][:num]
    thresholds = [0.3, 0.2, 0.2, 0.3, 0.25][:num]
    matchers, refs = [], []
    for g, full, threshold in zip(order, flags, thresholds):
        c, l = grids[g]
        matchers.append(_matcher(sm, c, l, 5, linear_search_window=window[0],
                                 angular_search_window=window[1]))
        om = _oracle(oracle, c, l, 5, *window)
        refs.append(om.match_full_submap(cloud, threshold) if full
                    else om.match(init, cloud, threshold))
    initial = [sm.Rigid2d(*init)] * num
    stats = []
    for dive in DIVES:
        debug(fast2d_dive=dive)
        found, scores, poses, st = sm.match_batch(matchers, initial, flags, thresholds, cloud)
        for k, ref in enumerate(refs):
            _same((found[k], scores[k], poses[k]), ref)
        stats.append(st)
    for key in ("coarse_candidates", "num_scans"):
        assert stats[0][key] == stats[1][key], key


def test_wave_dive_from_eight_threads(sm, oracle, big, debug):
    """Eight host threads issuing searches at once (the bench headline's shape), as
    test_queue_search_from_eight_threads does: every one equal to the oracle's."""
    cells, lim, _, scans = big
    om = _oracle(oracle, cells, lim, 7)
    refs = [om.match_full_submap(s, 0.6) for s in scans]
    gm = _matcher(sm, cells, lim, 7)
    clouds = [sm.PointCloudOnDevice(s) for s in scans]
    debug(fast2d_dive=2)

    def worker(t):
        out = []
        for j in range(10):
            k = (t + j) % len(scans)
            f, s, p, _ = sm.match_full_submap_batch([gm], clouds[k], 0.6)
            out.append((k, f[0], s[0], p[0]))
        return out
    with ThreadPoolExecutor(8) as pool:
        for results in pool.map(worker, range(8)):
            for k, f, s, p in results:
                _same((f, s, p), refs[k])


# ----------------------------------------------------------------------------
# The fused front end: cells, bounds and sums against the oracle
# ----------------------------------------------------------------------------
def _prepare_equals_the_oracle(sm, oracle, cells, lim, depth, cloud, init, window=()):
    om = _oracle(oracle, cells, lim, depth, *window)
    kw = dict(linear_search_window=window[0], angular_search_window=window[1]) if window else {}
    gm = _matcher(sm, cells, lim, depth, **kw)
    ref = om.prepare(list(init) if init else [0, 0, 0], cloud, init is None)
    got = gm.debug_prepare(sm.Rigid2d(*init) if init else None, cloud, init is None)
    assert got["num_scans"] == ref["num_scans"] and got["step"] == ref["step"]
    np.testing.assert_array_equal(got["scans"], ref["scans"])
    np.testing.assert_array_equal(got["bounds"], ref["bounds"])
    np.testing.assert_array_equal(got["sums"], ref["sums"])
    return om, gm


@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("group", [1, 2])
def test_fused_front_end_equals_the_oracle(sm, oracle, small, debug, group, n):
    """The introspection entry (exact sums: the ungrouped pass of the kernel), then a search on
    the same data with the group pass on or off; under group bounds the device checks every bound
    against the exact sums of its rotations (fast2d_group_verify = 1: a violation fails the call)."""
    cells, lim, world, scan = small
    cloud = np.ascontiguousarray(scan[:n])
    debug(fast2d_group=group)
    om, gm = _prepare_equals_the_oracle(sm, oracle, cells, lim, 5, cloud, None)
    truth = world.free_pose(5, 0.5)
    init = (truth[0] + 0.3, truth[1] - 0.2, truth[2] + 0.1)
    _prepare_equals_the_oracle(sm, oracle, cells, lim, 5, cloud, init, (2.0, math.radians(20.0)))
    debug(fast2d_group=group, fast2d_group_verify=1 if group == 2 else 0)
    _same(gm.match_full_submap(cloud, 0.3), om.match_full_submap(cloud, 0.3))


@pytest.mark.parametrize("group", [0, 1])
def test_fused_front_end_at_the_lds_edge(sm, oracle, synth, debug, group):
    """A depth-5 60 x 60 grid under 4000 points: three rotations' cells and the candidate sums
    come to the 64 KB a workgroup can have (the planner decides whether the group pass fits)."""
    cells, lim, world = synth.make_submap(19, 60, 60, 0.05, 5, 300, 30.0, 0.01)
    cloud = world.scan(world.free_pose(2, 0.3), 4000, 30.0, 0.01, 3)
    assert cloud.shape[0] == 4000
    debug(fast2d_group=group)
    om, gm = _prepare_equals_the_oracle(sm, oracle, cells, lim, 5, cloud, None)
    debug(fast2d_group=group, fast2d_group_verify=0 if group == 1 else 1)
    _same(gm.match_full_submap(cloud, 0.3), om.match_full_submap(cloud, 0.3))
