"""Ceres2DKernel<false> (csrc/ceres_2d.hip) and the 3D kernel (csrc/ceres_3d.hip) against the oracle
on the cases of tests/ceres_edge_cases.py: single Levenberg-Marquardt steps, grid borders, step
control and cloud sizes.  tests/test_ceres_edge_cases.py shows on the oracle alone that every case
reaches the branch it is named for and is stable, and measures the one-step tolerance.

Bars: the one_step cases hold the pose to that measured tolerance (1000 x the oracle's own spread
under reordered sums and an ulp of the angle, at most 1e-10), initial and final cost to 1e-9; all
other cases hold the project's whole-solve bar (_assert_ceres_close / _ceres3d_compare: pose 1e-6,
identical step counts and termination).  The resident-grid and batch entries must equal the
single call bit for bit: same kernel, same inputs.
"""
import math

import numpy as np
import pytest

import ceres_edge_cases as ec
from test_gpu_3d import _ceres3d_compare, _pose7
from test_gpu_r2_paths import _assert_ceres_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sm():
    from cartographer_amd import _lib, scan_matching
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching


@pytest.fixture(scope="module")
def sm3():
    from cartographer_amd import _lib, scan_matching_3d
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching_3d


@pytest.fixture(scope="module")
def tolerance(synth, oracle):
    return ec.one_step_tolerance(oracle, synth)


def _assert_one_step(got_pose, summary, ref, tolerance):
    """One iteration from the initial pose: the pose is a closed function of the cost, J^T r and
    J^T J there."""
    difference = float(np.abs(np.asarray(got_pose) - ref["pose"]).max())
    print("one-step device-to-oracle pose difference %.3g (tolerance %.3g)" % (difference, tolerance))
    assert difference <= tolerance
    assert abs(summary["initial_cost"] - ref["initial_cost"]) <= 1e-9 * max(1.0, ref["initial_cost"])
    assert abs(summary["final_cost"] - ref["final_cost"]) <= 1e-9 * max(1.0, ref["final_cost"])
    assert (summary["num_successful_steps"], summary["num_unsuccessful_steps"],
            summary["termination"]) == ec.counts(ref)


# ================================================================================ 2D ============
@pytest.fixture(scope="module")
def grids_2d(sm, synth):
    """The non-square submap as host cells and resident in HBM."""
    from cartographer_amd import grid_2d
    sc = ec.scene_2d(synth)
    lim = sc.lim
    host = sm.Grid2D(sc.cells, lim["resolution"], lim["max_x"], lim["max_y"])
    resident = grid_2d.ProbabilityGridOnDevice(ec.RES_2D, (lim["max_x"], lim["max_y"]), ec.NX_2D,
                                               ec.NY_2D, cells=sc.cells)
    return host, resident


def _xyt(pose):
    return (pose.x, pose.y, pose.theta)


@pytest.mark.parametrize("name", ec.NAMES_2D)
def test_ceres2d_edge_case_equals_the_oracle(sm, synth, oracle, grids_2d, tolerance, name):
    case = {c.name: c for c in ec.cases_2d(synth)}[name]
    host, resident = grids_2d
    ref = ec.oracle_2d(oracle, synth, case)
    w = case.weights
    m = sm.CeresScanMatcher2D(w[0], w[1], w[2], case.nonmonotonic, case.iterations)
    pose, summary = m.match(case.target, sm.Rigid2d(*case.init), case.cloud, host)
    print(name, summary, "oracle", ec.counts(ref),
          "pose difference %.3g" % np.abs(np.array(_xyt(pose)) - ref["pose"]).max())
    if case.family == "one_step":
        _assert_one_step(_xyt(pose), summary, ref, tolerance)
    else:
        _assert_ceres_close(pose, summary, ref)
    if case.steps == (0, 0):          # zero gradient: CONVERGENCE before the first iteration
        assert _xyt(pose) == tuple(case.init) and summary["termination"] == 0
    pose2, summary2 = m.match(case.target, sm.Rigid2d(*case.init), case.cloud, resident)
    assert _xyt(pose2) == _xyt(pose)
    assert summary2 == summary


def test_ceres2d_mixed_batch_equals_the_single_calls(sm, synth, oracle, grids_2d):
    """cmx_fast2d_refine_pairs indexes problems[blockIdx.x]: a border case, a one-point cloud, a
    cloud wholly outside (zero gradient), a solve that stops at the iteration cap and a pair
    without a search result in one launch, each bit for bit what its single call returns."""
    sc = ec.scene_2d(synth)
    host, _ = grids_2d
    table = {c.name: c for c in ec.cases_2d(synth)}
    picks = ["border_corner_minus_x_plus_y", "size_1", "border_all_outside_zero_gradient",
             "step_rejected_a_nonmonotonic", "size_257"]
    found = [1, 1, 1, 1, 0]
    clouds = [table[n].cloud for n in picks]
    poses = [sm.Rigid2d(*table[n].init) for n in picks]
    matcher = sm.FastCorrelativeScanMatcher2D(host, 4)
    ceres = sm.CeresScanMatcher2D(5.0, 1.0, 1.0, True, 3)
    refined, summaries = ceres.refine_pairs([matcher] * len(picks), found, poses, clouds)
    got = []
    for k, name in enumerate(picks):
        if not found[k]:
            assert _xyt(refined[k]) == _xyt(poses[k])
            one, summary = ceres.refine_batch([matcher], [0], [poses[k]], clouds[k])
            assert _xyt(one[0]) == _xyt(refined[k]) and summary[0] == summaries[k]
            continue
        # constraint_builder_2d.cc:245-249: the target is the pose's own translation
        single, summary = ceres.match(_xyt(poses[k])[:2], poses[k], clouds[k], host)
        assert _xyt(refined[k]) == _xyt(single), name
        assert summaries[k] == summary, name
        ref = oracle.ceres2d_match(sc.cells, ec.RES_2D, sc.lim["max_x"], sc.lim["max_y"],
                                   _xyt(poses[k])[:2], _xyt(poses[k]), clouds[k], 5.0, 1.0, 1.0,
                                   True, 3)
        _assert_ceres_close(refined[k], summary, ref)
        got.append(ec.counts(ref))
    assert got[1][0] >= 1                             # the one-point cloud moved
    assert got[2] == (0, 0, 0)                        # wholly outside: converged at once
    assert got[3] == (3, 0, 1)                        # stopped by the cap


# ================================================================================ 3D ============
@pytest.fixture(scope="module")
def resident_3d(synth):
    """{resolution: HybridGridOnDevice} of the scene's grids: the same scans inserted on the
    device and into synth.HybridGrid, whose voxel lists are the scene's."""
    from cartographer_amd import grid_3d
    sc = ec.scene_3d(synth)
    out = {}
    for resolution, voxels in ((0.1, sc.vox), (0.2, sc.mid_vox), (0.3, sc.low_vox)):
        dev, host = grid_3d.HybridGridOnDevice(resolution), synth.HybridGrid(resolution)
        for origin, returns in sc.inserts:
            dev.insert(origin, returns, 0.7, 0.4, 2)
            host.insert(origin, returns, 0.7, 0.4, 2)
        assert np.array_equal(host.voxels(), voxels)
        out[resolution] = dev
    return out


def _rigid3(sm3, init7):
    return sm3.Rigid3d(tuple(init7[:3]), tuple(init7[3:]))


@pytest.mark.parametrize("name", ec.NAMES_3D)
def test_ceres3d_edge_case_equals_the_oracle(sm3, synth, oracle, resident_3d, tolerance, name):
    case = {c.name: c for c in ec.cases_3d(synth, oracle)}[name]
    init = case.init7()
    pairs = list(case.pairs)
    m = sm3.CeresScanMatcher3D(list(case.weights), case.translation_weight, case.rotation_weight,
                               only_optimize_yaw=case.yaw_only,
                               use_nonmonotonic_steps=case.nonmonotonic,
                               max_num_iterations=case.iterations)
    if case.family == "one_step":
        ref = ec.oracle_3d(oracle, case)
        pose, summary = m.match(case.target, _rigid3(sm3, init), pairs)
        _assert_one_step(_pose7(pose), summary, ref, tolerance)
    else:
        ref, pose, summary = _ceres3d_compare(sm3, oracle, pairs, case.target, init,
                                              list(case.weights), case.translation_weight,
                                              case.rotation_weight, only_optimize_yaw=case.yaw_only,
                                              use_nonmonotonic_steps=case.nonmonotonic,
                                              max_num_iterations=case.iterations)
        assert summary["num_unsuccessful_steps"] == ref["num_unsuccessful_steps"]
    print(name, summary, "oracle", ec.counts(ref),
          "pose difference %.3g" % np.abs(_pose7(pose) - ref["pose"]).max())
    if case.steps == (0, 0):
        np.testing.assert_array_equal(_pose7(pose), init)
        assert summary["termination"] == 0
    if case.resident:
        on_device = [(p[0], resident_3d[p[1]]) for p in pairs]
        pose2, summary2 = m.match_grids(case.target, _rigid3(sm3, init), on_device)
        assert pose2 == pose and summary2 == summary


def test_ceres3d_more_than_three_pairs_is_an_invalid_argument(sm3, synth):
    from cartographer_amd._lib import CmxError, INVALID_ARGUMENT
    sc = ec.scene_3d(synth)
    m = sm3.CeresScanMatcher3D([1.0, 1.0, 1.0], 5.0, 4e2)
    m.options.num_pairs = 4                           # kMaxPairs is 3
    with pytest.raises(CmxError) as e:
        m.match((0, 0, 0), sm3.Rigid3d(), [(sc.lo, 0.3, sc.low_vox)] * 4)
    assert e.value.status == INVALID_ARGUMENT


def test_ceres3d_mixed_batch_equals_the_single_calls(sm3, synth, oracle):
    """cmx_fast3d_refine_pairs: a border case, a one-point node, a node wholly outside, a solve
    that stops at the iteration cap and a pair without a search result in one call, each bit for
    bit what cmx_ceres3d_match returns for it."""
    sc = ec.scene_3d(synth)
    table = {c.name: c for c in ec.cases_3d(synth, oracle)}
    hist = np.zeros(8, np.float32)
    matcher = sm3.FastCorrelativeScanMatcher3D(
        0.1, sc.vox, oracle.grid3d_size(0.1, sc.vox), 0.3, sc.low_vox, hist,
        branch_and_bound_depth=4, full_resolution_depth=2, min_rotational_score=0.0,
        min_low_resolution_score=0.2, linear_xy_search_window=1.0, linear_z_search_window=0.4,
        angular_search_window=math.radians(10.0))
    whole = sm3.TrajectoryNodeData(sc.hi, sc.lo, hist)
    one_point = ec.wall_first(sc)[:1]
    tiny = sm3.TrajectoryNodeData(one_point, one_point, hist)
    picks = [("border_minus_z", whole), ("size_1", tiny), ("border_all_outside", whole),
             ("step_cap_3", whole), ("border_plus_x", whole)]
    found = [True, True, True, True, False]
    poses = [_rigid3(sm3, table[n].init7()) for n, _ in picks]
    datas = [d for _, d in picks]
    ceres = sm3.CeresScanMatcher3D([1.0, 6.0], 0.01, 0.1, use_nonmonotonic_steps=True,
                                   max_num_iterations=3)
    refined, summaries = ceres.refine_pairs([matcher] * len(picks), found, poses, datas)
    got = []
    for k, (name, data) in enumerate(picks):
        if not found[k]:
            assert refined[k] == poses[k] and summaries[k]["num_successful_steps"] == 0
            continue
        pairs = [(data.high_resolution_point_cloud, 0.1, sc.vox),
                 (data.low_resolution_point_cloud, 0.3, sc.low_vox)]
        single, summary = ceres.match(poses[k].translation, poses[k], pairs)
        assert refined[k] == single, name
        assert summaries[k] == summary, name
        ref = oracle.ceres3d_match(pairs, poses[k].translation, table[name].init7(), [1.0, 6.0],
                                   translation_weight=0.01, rotation_weight=0.1,
                                   use_nonmonotonic_steps=True, max_num_iterations=3)
        np.testing.assert_allclose(_pose7(refined[k]), ref["pose"], rtol=0, atol=1e-6)
        assert (summary["num_successful_steps"], summary["num_unsuccessful_steps"],
                summary["termination"]) == ec.counts(ref), name
        got.append(ec.counts(ref))
    assert got[1][1] == 3                             # the one-point node: every step rejected
    assert got[2] == (0, 0, 0)                        # wholly outside: converged at once
    assert got[3] == (3, 0, 1)                        # stopped by the cap
