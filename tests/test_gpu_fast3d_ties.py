"""The exact tie resolution of the fast 3D search: distinct leaves tied for the best score.

A matcher of empty grids scores every candidate exactly 0.1 (kMinProbability), so with
min_score 0.05 nothing is pruned: the reference's depth-first search keeps the first leaf it meets,
the GPU search records every leaf, and the host has to repeat the reference's order (its std::sort
of the lowest-resolution candidates, then the descent) among all of them.  In every case the
winning translation differs from the initial one, so a tie rule that returns any other leaf shows.
"""
import numpy as np
import pytest

from test_gpu_3d import _assert_result, _assert_same_results, _fast3d_batch_scene
from test_oracle_reference_pins_3d import quat_from_angle_axis

pytestmark = pytest.mark.gpu

# (branch_and_bound_depth, full_resolution_depth, linear_xy, linear_z, angular, n_high)
CASES = [(3, 2, 0.4, 0.2, 0.2, 5), (2, 1, 0.3, 0.1, 0.1, 1), (4, 2, 0.8, 0.4, 0.3, 70)]
# Lowest-resolution candidates and the winning translation of each case on the CPU oracle.
EXPECTED = {CASES[0]: (90, (0.43, -0.38, -0.19)), CASES[1]: (96, (-0.27, 0.32, 0.11)),
            CASES[2]: (162, (0.03, 0.02, -0.39))}
INITIAL = (0.03, 0.02, 0.01)
IDENTITY = [0, 0, 0, 1, 0, 0, 0]
HIST = np.zeros(8, np.float32)
MIN_SCORE = 0.05


@pytest.fixture(scope="module")
def sm3():
    from cartographer_amd import _lib, scan_matching_3d
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching_3d


def _options(case):
    depth, frd, linear_xy, linear_z, angular, _ = case
    return dict(branch_and_bound_depth=depth, full_resolution_depth=frd, min_rotational_score=0.0,
                min_low_resolution_score=0.0, linear_xy_search_window=linear_xy,
                linear_z_search_window=linear_z, angular_search_window=angular)


def _clouds(case):
    n = case[5]
    hi = np.random.default_rng(3).uniform(-1, 1, (n, 3)).astype(np.float32)
    return hi, hi[:max(1, n // 3)].copy()


def _all_ties(sm3, oracle, case):
    """(GPU matcher of empty grids, its node data, the oracle's result) of one case."""
    from cartographer_amd._lib import VOXEL_DTYPE
    none = np.zeros(0, VOXEL_DTYPE)
    opt = _options(case)
    hi, lo = _clouds(case)
    om = oracle.FastCorrelativeScanMatcher3D(
        0.1, none, 0.1, none, HIST, opt["branch_and_bound_depth"], opt["full_resolution_depth"],
        opt["min_rotational_score"], opt["min_low_resolution_score"],
        opt["linear_xy_search_window"], opt["linear_z_search_window"],
        opt["angular_search_window"])
    ref = om.match(list(INITIAL) + [1, 0, 0, 0], IDENTITY, [1, 0, 0, 0], hi, lo, HIST, MIN_SCORE)
    gm = sm3.FastCorrelativeScanMatcher3D(0.1, none, 128, 0.1, none, HIST, **opt)
    return gm, sm3.TrajectoryNodeData(hi, lo, HIST), ref


@pytest.mark.parametrize("case", CASES, ids=lambda c: "depth%d_frd%d_n%d" % (c[0], c[1], c[5]))
def test_every_candidate_ties(sm3, oracle, case):
    gm, data, ref = _all_ties(sm3, oracle, case)
    coarse, winner = EXPECTED[case]
    assert ref["found"]
    assert np.float32(ref["score"]) == np.float32(0.1)
    assert ref["coarse_candidates"] == coarse
    np.testing.assert_allclose(ref["pose"][:3], winner, atol=1e-6)
    assert not np.allclose(ref["pose"][:3], INITIAL, atol=1e-3)
    got = gm.match(sm3.Rigid3d(INITIAL, (1, 0, 0, 0)), sm3.Rigid3d(), data, MIN_SCORE)
    _assert_result(ref, got)
    assert gm.last_stats["coarse_candidates"] == ref["coarse_candidates"]
    assert gm.last_stats["num_scans"] == ref["num_scans"]


def test_all_ties_pairs_inside_a_batch(sm3, oracle, synth):
    """One fast3d_match_pairs call: an ordinary found pair, then two all-ties pairs (the
    per-problem filter of the shared leaf list, a non-zero base of the lowest-resolution scores).
    Each pair's result equals its single call's."""
    matchers, pos, scene_data = _fast3d_batch_scene(sm3, synth, [5])
    ident = sm3.Rigid3d()
    node0 = sm3.Rigid3d(tuple(pos + np.array([0.3, -0.2, 0.1])),
                        tuple(quat_from_angle_axis(0.05, [0, 0, 1])))
    expected = [matchers[0].match(node0, ident, scene_data, 0.12)]
    assert expected[0] is not None
    datas, nodes, thresholds = [scene_data], [node0], [0.12]
    for case in (CASES[0], CASES[2]):
        gm, data, ref = _all_ties(sm3, oracle, case)
        node = sm3.Rigid3d(INITIAL, (1, 0, 0, 0))
        single = gm.match(node, ident, data, MIN_SCORE)
        _assert_result(ref, single)
        matchers.append(gm)
        datas.append(data)
        nodes.append(node)
        thresholds.append(MIN_SCORE)
        expected.append(single)
    got, _ = sm3.fast3d_match_pairs(matchers, nodes, [ident] * 3, [False] * 3, thresholds, datas)
    _assert_same_results(expected, got)
