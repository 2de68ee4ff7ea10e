"""Fast 2D batches of UNLIKE submaps: one call whose problems take different routes through the
front end (fast_2d_coarse.hip, PlanFrontEnd / PrepareAndScoreCoarse).

The front end decides per problem -- fused with group bounds, fused on the level itself, separate
launches over phase planes of 128 / 192 / 256 bytes, separate launches without planes -- and then
issues ONE launch per route whose parameters are maxima or "any" flags over the whole batch (the
accumulators and the LDS of the fused launch, its units, the rotations per launch, the dive's
grid).  Every other GPU test builds its batches from one recipe (400 x 400, depth 7), so that all
problems share a route and a size; here grids of 1 x 1 ... 400 x 400 cells, windowed and
full-submap searches, windows of 1 ... 450 rotations meet in one call.

Every case first reads the plan (cmx_debug_fast2d_plan, the function the launch path itself asks)
and asserts that the intended mix is there; then every pair of the batch is compared with
  (a) the oracle's FastCorrelativeScanMatcher2D on that pair, and
  (b) the same matcher's single match / match_full_submap call.
Bars as in test_gpu_2d.py: found flag equal, f32 score bit-equal, pose to 1e-12 (f64 from integer
offsets), lowest-resolution candidate counts equal.
"""
import math
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES = 0.05
# name -> (seed, num_x_cells, num_y_cells) of synth.make_submap; "g1" is a single occupied cell
GRIDS = {
    "g60": (11, 60, 60), "g60b": (12, 60, 60), "g100": (11, 100, 100), "g100b": (12, 100, 100),
    "g110": (11, 110, 110), "g170": (11, 170, 170), "g200": (11, 200, 200),
    "g97x233": (11, 97, 233), "g400": (11, 400, 400), "g400x120": (11, 400, 120),
    "g33x200": (11, 33, 200),
}

# One (scan, submap) pair of a batch: the matcher (grid, depth, windows), windowed (around the
# scan's true pose + offset) or full-submap, and its acceptance threshold.
Pair = namedtuple("Pair", "grid depth lin ang full min_score offset")


def W(grid, depth, lin, ang, min_score=0.2, offset=(0.1, -0.05, 0.02)):
    return Pair(grid, depth, lin, ang, 0, min_score, offset)


def F(grid, depth, min_score=0.2, lin=7.0, ang=math.radians(30.0)):
    return Pair(grid, depth, lin, ang, 1, min_score, (0.0, 0.0, 0.0))


@pytest.fixture(scope="module")
def sm():
    from cartographer_amd import _lib, scan_matching
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching


class Zoo:
    """Grids, clouds, matchers and per-pair reference results, each made once per module: what a
    pair returns does not depend on the batch it travels in (that is the claim under test)."""

    def __init__(self, sm, oracle, synth):
        self.sm, self.oracle, self.synth = sm, oracle, synth
        self._grids, self._matchers, self._oracles, self._refs, self._singles = {}, {}, {}, {}, {}
        _, _, world = self._submap("g100")
        self.truth = world.free_pose(3, 0.3)
        scan = world.scan(self.truth, 300, 5.0, 0.01, 1)
        assert 64 <= len(scan) <= 400
        # the LDS case: 4000 points (n_pad = 4032), the farthest 388 cells away
        _, _, small = self._submap("g60")
        self.truth_big = small.free_pose(3, 0.3)
        dense = small.scan(self.truth_big, 4200, 5.0, 0.01, 1)[:3999]
        assert len(dense) == 3999 and np.hypot(dense[:, 0], dense[:, 1]).max() < 19.0
        far = np.array([[388 * RES * math.cos(0.7), 388 * RES * math.sin(0.7), 0.0]], np.float32)
        rng = np.random.default_rng(4)
        outside = np.zeros((128, 3), np.float32)
        outside[:, :2] = rng.uniform(2.0, 4.0, (128, 2))
        self.clouds = {"scan": scan, "big": np.concatenate([dense, far]), "outside": outside}
        self.truths = {"scan": self.truth, "big": self.truth_big, "outside": np.zeros(3)}

    def _submap(self, name):
        if name not in self._grids:
            if name == "g1":
                cells = np.full((1, 1), 3000, np.uint16)
                self._grids[name] = (cells, dict(resolution=RES, max_x=RES, max_y=RES), None)
            else:
                seed, nx, ny = GRIDS[name]
                self._grids[name] = self.synth.make_submap(seed, nx, ny, RES, 12, 400, 5.0, 0.01)
        return self._grids[name]

    def initial(self, pair, cloud):
        return [float(t + o) for t, o in zip(self.truths[cloud], pair.offset)]

    def matcher(self, pair):
        key = pair[:4]
        if key not in self._matchers:
            cells, lim, _ = self._submap(pair.grid)
            grid = self.sm.Grid2D(cells, RES, lim["max_x"], lim["max_y"])
            self._matchers[key] = self.sm.FastCorrelativeScanMatcher2D(grid, pair.depth, pair.lin,
                                                                       pair.ang)
        return self._matchers[key]

    def reference(self, pair, cloud):
        """(a): the oracle on this pair."""
        key = (pair, cloud)
        if key not in self._refs:
            if pair[:4] not in self._oracles:
                cells, lim, _ = self._submap(pair.grid)
                self._oracles[pair[:4]] = self.oracle.FastCorrelativeScanMatcher2D(
                    cells, RES, lim["max_x"], lim["max_y"], pair.depth, pair.lin, pair.ang)
            om = self._oracles[pair[:4]]
            xyz = self.clouds[cloud]
            self._refs[key] = (om.match_full_submap(xyz, pair.min_score) if pair.full else
                               om.match(self.initial(pair, cloud), xyz, pair.min_score))
        return self._refs[key]

    def single(self, pair, cloud):
        """(b): the matcher's single call (default switches), as (found, score, pose, stats)."""
        key = (pair, cloud)
        if key not in self._singles:
            gm, xyz = self.matcher(pair), self.clouds[cloud]
            got = (gm.match_full_submap(xyz, pair.min_score) if pair.full else
                   gm.match(self.sm.Rigid2d(*self.initial(pair, cloud)), xyz, pair.min_score))
            self._singles[key] = got + (dict(gm.last_stats),)
        return self._singles[key]

    def plan(self, pairs, cloud):
        return self.sm.debug_plan([self.matcher(p) for p in pairs], [p.full for p in pairs],
                                  self.clouds[cloud])

    def batch(self, pairs, cloud):
        return self.sm.match_batch([self.matcher(p) for p in pairs],
                                   [self.sm.Rigid2d(*self.initial(p, cloud)) for p in pairs],
                                   [p.full for p in pairs], [p.min_score for p in pairs],
                                   self.clouds[cloud])


@pytest.fixture(scope="module")
def zoo(sm, oracle, synth):
    return Zoo(sm, oracle, synth)


def _xyt(pose):
    return [pose.x, pose.y, pose.theta]


def _check_batch(zoo, debug, pairs, cloud, **switches):
    """The batch under `switches` against (a) and (b) of every pair; returns the batch's output."""
    from cartographer_amd import _lib
    _lib.debug_reset()
    refs = [zoo.reference(p, cloud) for p in pairs]
    singles = [zoo.single(p, cloud) for p in pairs]
    debug(**switches)
    found, scores, poses, stats = zoo.batch(pairs, cloud)
    for k, (ref, one) in enumerate(zip(refs, singles)):
        where = f"pair {k} ({pairs[k]})"
        assert bool(found[k]) == bool(ref["found"]) == bool(one[0]), where
        assert one[3]["coarse_candidates"] == ref["coarse_candidates"], where
        if not ref["found"]:
            continue
        assert np.float32(scores[k]) == np.float32(ref["score"]) == np.float32(one[1]), where
        np.testing.assert_allclose(_xyt(poses[k]), ref["pose"], rtol=0, atol=1e-12, err_msg=where)
        np.testing.assert_allclose(_xyt(poses[k]), _xyt(one[2]), rtol=0, atol=1e-12, err_msg=where)
    assert stats["coarse_candidates"] == sum(r["coarse_candidates"] for r in refs)
    assert stats["num_scans"] == sum(r["num_scans"] for r in refs)
    return found, scores, poses, stats


# ----------------------------------------------------------------------------
# Case 1: the LDS budget of the fused launch
# ----------------------------------------------------------------------------
# 4000 points, depth 5, a window of 25 m and 9 rotations: the 60 x 60 grid (A) asks for 62^2
# accumulators and is grouped on its own (12 * 4032 + 4 * (128 + 3844) + 1024 = 65 296 B), the
# 100 x 100 grid (B) for 70^2, fused but too large for three scans of points.  Their launch was
# sized from "any problem grouped" and "the largest accumulators": 12 * 4032 + 4 * (128 + 4900) +
# 1024 = 69 520 B, above the 65 536 B a launch gets -- the whole call failed.
LDS_A = W("g60", 5, 25.0, 0.01, 0.1, (0.1, -0.05, 0.003))
LDS_B = W("g100", 5, 25.0, 0.01, 0.1, (0.1, -0.05, 0.003))
LDS_LIMIT = 64 * 1024


def _former_lds(problems, n):
    """What the launch asked for before it was checked against the limit."""
    n_pad = (n + 63) // 64 * 64
    fused = [q for q in problems if q["use_fused"]]
    group = 3 if any(q["group"] > 1 for q in fused) else 1
    return 4 * n_pad * group + 4 * (128 + max(q["acc"] for q in fused)) + 1024


def test_lds_plan_of_the_two_problems_alone_and_together(zoo):
    (a,), alone_a = zoo.plan([LDS_A], "big")
    (b,), alone_b = zoo.plan([LDS_B], "big")
    assert (a["use_fused"], a["group"], a["acc"], a["num_scans"]) == (1, 3, 62 * 62, 9)
    assert (b["use_fused"], b["group"], b["acc"], b["num_scans"]) == (1, 1, 70 * 70, 9)
    assert alone_a["fused_lds"] == 65296 and alone_a["any_group"] == 1 and alone_a["per_unit"] == 3
    assert alone_b["fused_lds"] == 37264 and alone_b["any_group"] == 0
    for pairs in ([LDS_A, LDS_B], [LDS_B, LDS_A]):
        problems, launch = zoo.plan(pairs, "big")
        # the sizes the two would have been launched with: over the limit ...
        assert _former_lds([a, b], 4000) == 69520 > LDS_LIMIT
        # ... so nobody is grouped, and the launch fits
        assert [q["group"] for q in problems] == [1, 1] and launch["any_group"] == 0
        assert launch["fused_acc"] == 70 * 70 and launch["fused_lds"] == 37264 <= LDS_LIMIT


@pytest.mark.parametrize("order", ["AB", "BA"])
def test_lds_budget_pair(zoo, debug, order):
    pairs = [LDS_A, LDS_B] if order == "AB" else [LDS_B, LDS_A]
    found, _, _, _ = _check_batch(zoo, debug, pairs, "big")
    assert found[pairs.index(LDS_A)] == 1           # (the scan was taken in A's world)


def test_lds_budget_pair_inside_a_batch_of_six(zoo, debug):
    """num >= 4: the scans' cells are stored and the tree is walked level by level."""
    others = [W(g, 5, 25.0, 0.01, 0.1, (0.1, -0.05, 0.003)) for g in ("g60b", "g100b", "g110", "g97x233")]
    pairs = [others[0], LDS_A, others[1], others[2], LDS_B, others[3]]
    alone = [zoo.plan([p], "big")[0][0] for p in pairs]
    assert [q["group"] for q in alone] == [3, 3, 1, 1, 1, 1] and _former_lds(alone, 4000) > LDS_LIMIT
    problems, launch = zoo.plan(pairs, "big")
    assert _routes(problems) == ["fused"] * 5 + ["generic"]
    assert launch["fused_lds"] <= LDS_LIMIT and launch["any_group"] == 0
    _check_batch(zoo, debug, pairs, "big")


# ----------------------------------------------------------------------------
# Case 2: grouped and ungrouped fused problems in one launch, within the budget
# ----------------------------------------------------------------------------
# g100: the level dilated by two cells fits its phase planes -- group bounds; g110: it does not
# (125 + 4 > 8 * 16 cells) -- every rotation on the level itself; one rotation only: nothing to
# group.  Different windows: different accumulators, different numbers of rotations.
GROUP_MIX = [W("g100", 5, 1.0, 0.06), W("g110", 5, 3.0, 0.02), W("g100b", 5, 2.0, 0.0),
             F("g60", 5, 0.3), W("g60b", 5, 0.5, 0.2, 0.05)]


@pytest.mark.parametrize("verify", [1, 3])
def test_grouped_and_ungrouped_fused_problems_share_a_launch(zoo, debug, verify):
    """fast2d_group_verify = 1: the device compares every group bound with the exact sums of its
    rotations, both launched with the accumulators of the largest problem; 3: and every unit as
    if its premise had failed."""
    problems, launch = zoo.plan(GROUP_MIX, "scan")
    assert all(q["use_fused"] for q in problems)
    assert [q["group"] for q in problems] == [3, 1, 1, 3, 3]
    assert len({q["acc"] for q in problems}) == 5 and len({q["num_scans"] for q in problems}) == 5
    assert problems[2]["num_scans"] == 1
    assert launch["any_group"] == 1 and launch["per_unit"] == 1
    assert launch["fused_acc"] == max(q["acc"] for q in problems) > problems[0]["acc"]
    assert launch["max_scans"] == problems[3]["num_scans"] > 100
    _check_batch(zoo, debug, GROUP_MIX, "scan", fast2d_group_verify=verify)
    # two problems, both grouped: units of three rotations (per_unit 3), the work-queue search
    both = [GROUP_MIX[0], GROUP_MIX[4]]
    assert zoo.plan(both, "scan")[1]["per_unit"] == 3
    _check_batch(zoo, debug, both, "scan", fast2d_group_verify=verify)


# ----------------------------------------------------------------------------
# Case 3: all four routes in one call
# ----------------------------------------------------------------------------
# At depth 5 (16-cell lattice blocks): 400 x 400 has no phase planes (27 x 27 cells per plane) ->
# generic; 200 x 200 planes of 256 bytes, 170 x 170 of 192, 97 x 233 of 128; 110 x 110 fused on
# the level itself, 100 x 100 fused with group bounds.  Windowed and full-submap, thresholds of
# their own, one pair that finds nothing.
ALL_ROUTES = [F("g400", 5, 0.3), W("g97x233", 5, 2.0, 0.3, 0.25), F("g100", 5, 0.4),
              W("g170", 5, 1.5, 0.2, 0.1), F("g200", 5, 0.99), W("g110", 5, 1.0, 0.1, 0.15)]


def _routes(problems):
    out = []
    for q in problems:
        if q["use_fused"]:
            out.append("fused+group" if q["group"] > 1 else "fused")
        else:
            out.append(f"planes{q['plane_stride']}" if q["use_planes"] else "generic")
    return out


def test_all_routes_in_one_call(zoo, debug):
    problems, launch = zoo.plan(ALL_ROUTES, "scan")
    assert _routes(problems) == ["generic", "planes128", "fused+group", "planes192", "planes256",
                                 "fused"]
    assert launch["any_group"] == 1 and launch["per_unit"] == 1
    assert launch["plane_acc_cells"] > launch["fused_acc"] > 0
    fused = _check_batch(zoo, debug, ALL_ROUTES, "scan")
    assert fused[0][2] == 1 and fused[0][4] == 0          # (the scan's own submap; nothing reaches 0.99)
    # the same call with every problem on the separate launches: the same constraint list
    debug(fast2d_unfused=1)
    problems, _ = zoo.plan(ALL_ROUTES, "scan")
    assert _routes(problems) == ["generic", "planes128", "planes64", "planes192", "planes256",
                                 "planes64"]
    unfused = zoo.batch(ALL_ROUTES, "scan")
    np.testing.assert_array_equal(fused[0], unfused[0])
    np.testing.assert_array_equal(fused[1][fused[0] != 0], unfused[1][unfused[0] != 0])
    for a, b, ok in zip(fused[2], unfused[2], fused[0]):
        assert not ok or _xyt(a) == _xyt(b)
    assert fused[3]["coarse_candidates"] == unfused[3]["coarse_candidates"]


def test_depths_do_not_mix_in_one_call(zoo, sm):
    """400 x 400 at depths 7, 6, 5 and 1 next to 97 x 233: the front end has a route for each
    (fused with and without group bounds, planes of 256 bytes, twice the generic kernel), but the tree search
    walks a batch level by level -- matchers of one call share branch_and_bound_depth, by design.
    The call says so before it launches anything."""
    from cartographer_amd._lib import CmxError
    pairs = [F("g400", 7), F("g400", 6), W("g400", 5, 2.0, 0.2), W("g400", 1, 0.5, 0.05),
             W("g97x233", 6, 2.0, 0.3)]
    problems, _ = zoo.plan(pairs, "scan")
    assert _routes(problems) == ["fused+group", "planes256", "generic", "generic", "fused"]
    with pytest.raises(CmxError, match="share branch_and_bound_depth"):
        zoo.batch(pairs, "scan")
    _, score, _ = zoo.matcher(pairs[0]).match_full_submap(zoo.clouds["scan"], 0.2)[:3]
    assert score is not None                      # (the library goes on working after the refusal)


# ----------------------------------------------------------------------------
# Case 4: non-square and tiny grids next to a large one
# ----------------------------------------------------------------------------
def _odd_shapes(depth, full_large):
    large = F("g400", depth, 0.3) if full_large else W("g400", depth, 1.0, 0.1)
    narrow = F("g33x200", depth, 0.1) if full_large else W("g33x200", depth, 2.0, 0.3, 0.1)
    return [large, W("g400x120", depth, 1.5, 0.2), narrow,
            W("g1", depth, 1.0, 0.1, 0.05, (0.3, 0.2, 0.0))]


def test_odd_shapes_at_depth_7(zoo, debug):
    pairs = _odd_shapes(7, True)
    problems, launch = zoo.plan(pairs, "scan")
    # (1 x 1: the level dilated by two cells does not fit its one lattice cell of 64)
    assert _routes(problems) == ["fused+group", "fused+group", "fused+group", "fused"]
    assert launch["fused_acc"] == problems[0]["acc"] > 10 * problems[3]["acc"]
    _check_batch(zoo, debug, pairs, "scan")
    _check_batch(zoo, debug, pairs, "scan", fast2d_group_verify=1)


def test_odd_shapes_at_depth_3(zoo, debug):
    pairs = _odd_shapes(3, False)
    problems, _ = zoo.plan(pairs, "scan")
    assert _routes(problems) == ["generic", "generic", "generic", "fused"]
    _check_batch(zoo, debug, pairs, "scan")


@pytest.mark.parametrize("depth", [7, 3])
def test_a_cloud_outside_the_smallest_grid(zoo, debug, depth):
    """128 points 2 - 4 m from the sensor, the 1 x 1 grid at the sensor, a window of 1 m: no
    candidate brings a point into the grid (the reference scores the floor value everywhere and
    returns its first candidate); the other grids of the batch see some of the points."""
    pairs = [W("g1", depth, 1.0, 0.1, 0.05, (0.0, 0.0, 0.0)), W("g400", depth, 1.0, 0.1, 0.05, (5.0, 5.0, 0.3)),
             W("g33x200", depth, 1.0, 0.1, 0.05, (1.0, 1.0, 0.0)),
             W("g400x120", depth, 1.0, 0.1, 0.05, (4.0, 2.0, -0.2))]
    problems, _ = zoo.plan(pairs, "outside")
    assert len(set(_routes(problems))) >= 2
    _check_batch(zoo, debug, pairs, "outside")


# ----------------------------------------------------------------------------
# Case 5: order independence
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_order_of_the_problems_changes_nothing(zoo, debug, where):
    """Case 3's batch with the problem of the largest accumulators first, in the middle, last."""
    problems, _ = zoo.plan(ALL_ROUTES, "scan")
    largest = int(np.argmax([q["acc"] if q["use_planes"] else -1 for q in problems]))
    rest = [k for k in range(len(ALL_ROUTES)) if k != largest]
    rest = rest[::-1] if where == "middle" else rest[1:] + rest[:1]
    at = {"first": 0, "middle": 3, "last": len(rest)}[where]
    order = rest[:at] + [largest] + rest[at:]
    assert sorted(order) == list(range(len(ALL_ROUTES))) and order.index(largest) == at
    pairs = [ALL_ROUTES[k] for k in order]
    permuted, _ = zoo.plan(pairs, "scan")
    assert permuted == [problems[k] for k in order]
    _check_batch(zoo, debug, pairs, "scan")     # per pair: the same references, wherever it stands


# ----------------------------------------------------------------------------
# Case 6: batch sizes across the num >= 4 switch
# ----------------------------------------------------------------------------
UNLIKE = [ALL_ROUTES[2], ALL_ROUTES[5], ALL_ROUTES[3], ALL_ROUTES[1], ALL_ROUTES[4],
          W("g60", 5, 0.8, 0.15), ALL_ROUTES[0]]


@pytest.mark.parametrize("num", [2, 3, 4, 7])
def test_batch_sizes_of_unlike_matchers(zoo, debug, num):
    """Up to three problems keep the scans on chip and take the work-queue search, from four on
    the cells are stored and the tree is walked level by level: same results."""
    pairs = UNLIKE[:num]
    problems, _ = zoo.plan(pairs, "scan")
    assert len(set(_routes(problems))) == min(num, 6)
    _check_batch(zoo, debug, pairs, "scan")
