"""The lean chain step of the work-queue tree search (fast_2d_queue.hip, TreeQueueKernel<0>; debug switch
fast2d_chain = 0, the default) against the step that waits for the bound wherever it uses it
(TreeQueueKernel<1>, fast2d_chain = 1: the kernel as it was) and against the oracle.  The lean step
picks the best node of a list round before it looks at the bound, decides about the round and the
node on one load of it, and loads the bound of a chain step with the level's first gathers, so
`keep` sees a bound that is a trip older.  None of that may change a result: every case runs under
both switch values and is compared with the oracle, in every shape the queue takes (one workgroup,
where almost every pop is a home pop; more wavefronts than sub-queues; thieves that give up at
once; sub-queues that overflow into the level path and its strict retry; a batch; eight threads).
Bars as in test_gpu_queue.py: found flag and f32 score bit-equal, pose to 1e-12 (f64 from integer
offsets).

`nodes_expanded` and `candidates_scored` depend on when a wavefront sees the bound rise, so they
are compared between the two switch values only where the bound is final before the tree search
starts: the grid of equal cells (every candidate has the dive's score) and bench.py's scan #0 under
exact lowest-resolution scores (its dive finds the optimum: 3 076 expansions on every path).
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAINS = (0, 1)     # the lean step, the one that waits for the bound wherever it uses it


@pytest.fixture(scope="module")
def sm():
    from cartographer_amd import _lib, scan_matching
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching


@pytest.fixture(scope="module")
def small(synth):
    """The `small` recipe of test_gpu_fast2d_wave_dive.py: a 100 x 100 grid and a scan of 1100
    points of it (cases take the first n)."""
    cells, lim, world = synth.make_submap(11, 100, 100, 0.05, 8, 400, 30.0, 0.01)
    scan = world.scan(world.free_pose(5, 0.5), 1100, 30.0, 0.01, 2)
    assert scan.shape[0] == 1100
    return cells, lim, world, scan


@pytest.fixture(scope="module")
def small700(small, oracle):
    """700 points of it at depth 5, with the oracle's full-submap result (shared by the cases that
    only change the shape of the queue)."""
    cells, lim, _, scan = small
    cloud = np.ascontiguousarray(scan[:700])
    ref = _oracle(oracle, cells, lim, 5).match_full_submap(cloud, 0.3)
    assert ref["found"]
    return cells, lim, cloud, ref


@pytest.fixture(scope="module")
def odd(synth):
    """37 x 53: divides nothing."""
    cells, lim, world = synth.make_submap(13, 37, 53, 0.05, 4, 200, 30.0, 0.01)
    scan = world.scan(world.free_pose(3, 0.3), 300, 30.0, 0.01, 4)
    return cells, lim, world, scan


@pytest.fixture(scope="module")
def big(synth, oracle):
    """bench.py's C2 world (400 x 400, depth 7), the first two scans of its headline and the
    oracle's results for them."""
    cells, lim, world = synth.make_submap(42, 400, 400, 0.05, 30, 1000, 30.0, 0.01)
    scans = [world.scan(world.free_pose(1234 + k, 0.5), 1000, 30.0, 0.01, 7 + k) for k in range(2)]
    om = _oracle(oracle, cells, lim, 7)
    with ThreadPoolExecutor(2) as pool:
        refs = list(pool.map(lambda s: om.match_full_submap(s, 0.6), scans))
    return cells, lim, scans, refs


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


def _both_chains(debug, gm, run, ref, counted=False, **switches):
    """run() under either chain step: equal to the oracle's `ref`; with `counted` the work counters
    of the two equal too.  Returns the statistics of the lean one."""
    stats = []
    for chain in CHAINS:
        debug(fast2d_chain=chain, **switches)
        _same(run(), ref)
        stats.append(dict(gm.last_stats))
    lean, waits = stats
    print("nodes_expanded lean / waiting:", lean["nodes_expanded"], waits["nodes_expanded"])
    print("candidates_scored lean / waiting:", lean["candidates_scored"], waits["candidates_scored"])
    for key in ("coarse_candidates", "num_scans") + (
            ("nodes_expanded", "candidates_scored") if counted else ()):
        assert lean[key] == waits[key], key
    return lean


# 64 | 65, 256 | 257 and 512 | 513: the gathers of 4, 8 and 16 cells a lane; 256 | 257: the first
# size at which an expansion can end after its first 256 points; 1024: the last size a wavefront
# holds
@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 512, 513, 1024])
@pytest.mark.parametrize("depth", [4, 5])
def test_lean_chain_point_counts(sm, oracle, small, debug, n, depth):
    cells, lim, _, scan = small
    cloud = np.ascontiguousarray(scan[:n])
    ref = _oracle(oracle, cells, lim, depth).match_full_submap(cloud, 0.3)
    gm = _matcher(sm, cells, lim, depth)
    _both_chains(debug, gm, lambda: gm.match_full_submap(cloud, 0.3), ref)


@pytest.mark.parametrize("depth", [2, 5])
def test_lean_chain_on_a_grid_that_divides_nothing(sm, oracle, odd, debug, depth):
    """Depth 2: the first expansion of a chain already scores leaves (nothing is ever pushed);
    depth 5 under group bounds."""
    cells, lim, _, scan = odd
    ref = _oracle(oracle, cells, lim, depth).match_full_submap(scan, 0.3)
    gm = _matcher(sm, cells, lim, depth)
    _both_chains(debug, gm, lambda: gm.match_full_submap(scan, 0.3), ref)


@pytest.mark.parametrize("switches", [
    {"fast2d_queue_blocks": 1},        # four wavefronts: almost every pop a home pop
    {"fast2d_queue_blocks": 2048},     # more wavefronts than sub-queues: pops are steals
    {"fast2d_queue_lost": 1},          # a thief leaves at its first lost race
    {"fast2d_queue_capacity": 2},      # sub-queues overflow: the level path takes over
    {"fast2d_queue_capacity": 2, "frontier_capacity": 4096},   # ... and overflows too: the strict retry
], ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
def test_lean_chain_in_every_shape_of_the_queue(sm, small700, debug, switches):
    cells, lim, cloud, ref = small700
    gm = _matcher(sm, cells, lim, 5)
    _both_chains(debug, gm, lambda: gm.match_full_submap(cloud, 0.3), ref, **switches)


@pytest.mark.parametrize("group", [1, 2], ids=["ungrouped", "grouped"])
@pytest.mark.parametrize("n", [1, 300])
def test_lean_chain_all_ties(sm, oracle, debug, n, group):
    """A grid of unknown cells, windowed (7 cells, 30 degrees: children beyond the bounds at every
    level): every candidate ties, every child is kept and up to three siblings are pushed at every
    step.  The bound is final from the first dive on, so a bound that is a trip older prunes the
    same: the work counters of the two steps are equal."""
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
    ref = om.match([4.0, 5.0, 0.0], cloud, 0.0)
    _both_chains(debug, gm, lambda: gm.match(sm.Rigid2d(4.0, 5.0, 0.0), cloud, 0.0), ref,
                 counted=True, fast2d_group=group)


def test_lean_chain_on_the_bench_world(sm, big, debug):
    """400 x 400 at depth 7, scans #0 and #1 as shipped; then scan #0 with exact lowest-resolution
    scores, where the dive finds the optimum and every path expands exactly the 3 076 nodes that
    reach the final bound."""
    cells, lim, scans, refs = big
    gm = _matcher(sm, cells, lim, 7)
    for scan, ref in zip(scans, refs):
        assert ref["found"]
        _both_chains(debug, gm, lambda: gm.match_full_submap(scan, 0.6), ref)
    exact = _both_chains(debug, gm, lambda: gm.match_full_submap(scans[0], 0.6), refs[0],
                         counted=True, fast2d_group=1)
    assert exact["nodes_expanded"] == 3076


def test_lean_chain_for_a_batch_of_unlike_submaps(sm, oracle, synth, small, odd, debug):
    """cmx_fast2d_match_batch over three unlike submaps, full and windowed searches mixed: the
    queue takes up to three problems, so a wavefront meets nodes of several problems, each with
    a bound of its own (a list round is then never dropped on the bound of problem 0)."""
    cells, lim, world, scan = small
    cloud = np.ascontiguousarray(scan[:600])
    grids = [(cells, lim), odd[:2], synth.make_submap(17, 160, 120, 0.05, 10, 400, 30.0, 0.01)[:2]]
    window = (1.0, math.radians(20.0))
    truth = world.free_pose(5, 0.5)
    init = [truth[0] + 0.2, truth[1] - 0.1, truth[2] + 0.05]
    flags = [1, 1, 0]
    thresholds = [0.3, 0.2, 0.2]
    matchers, refs = [], []
    for (c, l), full, threshold in zip(grids, flags, thresholds):
        matchers.append(_matcher(sm, c, l, 5, linear_search_window=window[0],
                                 angular_search_window=window[1]))
        om = _oracle(oracle, c, l, 5, *window)
        refs.append(om.match_full_submap(cloud, threshold) if full
                    else om.match(init, cloud, threshold))
    initial = [sm.Rigid2d(*init)] * 3
    stats = []
    for chain in CHAINS:
        debug(fast2d_chain=chain)
        found, scores, poses, st = sm.match_batch(matchers, initial, flags, thresholds, cloud)
        for k, ref in enumerate(refs):
            _same((found[k], scores[k], poses[k]), ref)
        stats.append(st)
    for key in ("coarse_candidates", "num_scans"):
        assert stats[0][key] == stats[1][key], key


def test_lean_chain_from_eight_threads(sm, small700, debug):
    """Eight host threads x ten searches at once, under either step: every result the oracle's."""
    cells, lim, cloud, ref = small700
    gm = _matcher(sm, cells, lim, 5)
    on_device = sm.PointCloudOnDevice(cloud)

    def worker(_):
        return [sm.match_full_submap_batch([gm], on_device, 0.3)[:3] for _ in range(10)]
    for chain in CHAINS:
        debug(fast2d_chain=chain)
        with ThreadPoolExecutor(8) as pool:
            for results in pool.map(worker, range(8)):
                for f, s, p in results:
                    _same((f[0], s[0], p[0]), ref)
