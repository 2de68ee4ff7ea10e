"""CeresScanMatcher2D::Match on a TSDF2D (cartographer_amd/csrc/ceres_2d.hip, the GridType::TSDF
case): TSDFMatchCostFunction2D's residuals and Jacobians, and whole solves with host planes,
resident planes and the batch entry.

The yardstick is tests/golden/ceres2d_tsdf_golden.npz, made by the reference's own cost function
and CeresScanMatcher2D::Match over the stand-in solver (make_ceres2d_tsdf_golden.py).  The solve
bar is test_gpu_r2_paths.py's _assert_ceres_close: pose within 1e-6, initial cost within 1e-9
and final cost within 1e-7 (relative above 1), the same termination and step counts.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import make_ceres2d_tsdf_golden as mk  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "ceres2d_tsdf_golden.npz")))


@pytest.fixture(scope="module")
def insert_golden():
    return dict(np.load(mk.INSERT_GOLDEN))


@pytest.fixture(scope="module")
def sm():
    from cartographer_amd import scan_matching
    return scan_matching


def _host(sm, grid):
    tsd, wgt, res, mx, my, trunc, maxw = grid
    return sm.TSDF2D(tsd, wgt, res, mx, my, trunc, maxw)


def _device(grid, device=0):
    from cartographer_amd import grid_2d
    tsd, wgt, res, mx, my, trunc, maxw = grid
    return grid_2d.TSDF2DOnDevice(res, (mx, my), tsd.shape[1], tsd.shape[0], trunc, maxw,
                                  tsd_cells=tsd, weight_cells=wgt, device=device)


def _residual_cases():
    g = np.load(os.path.join(GOLDEN, "ceres2d_tsdf_golden.npz"))
    return sorted({k.split("/")[1] for k in g.files if k.startswith("res/")})


def _solve_cases():
    g = np.load(os.path.join(GOLDEN, "ceres2d_tsdf_golden.npz"))
    return sorted({k.split("/")[1] for k in g.files if k.startswith("solve/")})


@pytest.mark.parametrize("case", _residual_cases())
def test_residuals_match_the_reference(sm, golden, insert_golden, case):
    key = f"res/{case}"
    grid = _host(sm, mk.grid_of(golden, insert_golden, str(golden[key + "/grid"])))
    scaling = float(golden[key + "/scaling"])
    poses, clouds = golden[key + "/poses"], golden[key + "/xyz"]
    for p in range(poses.shape[0]):
        valid, r, J = sm.tsdf_match_residuals(grid, scaling, poses[p], clouds[p])
        assert valid == bool(golden[key + "/valid"][p]), (case, p)
        if not valid:
            continue
        ref_r, ref_J = golden[key + "/residuals"][p], golden[key + "/jacobian"][p]
        assert np.all(np.abs(r - ref_r) <= 1e-10 * np.maximum(1.0, np.abs(ref_r))), (case, p)
        assert np.all(np.abs(J - ref_J) <= 1e-10 * np.maximum(1.0, np.abs(ref_J))), (case, p)


def test_reference_unit_test_expectations(sm, golden, insert_golden):
    """tsdf_match_cost_function_2d_test.cc's own expectations, on the device."""
    grid = _host(sm, mk.grid_of(golden, insert_golden, "ref_fixture"))
    cloud = np.array([[0.0, 1.0, 0.0]], np.float32)
    for y, expected in ((0.0, 0.0), (0.1, -0.1), (-0.1, 0.1)):
        valid, r, J = sm.tsdf_match_residuals(grid, 1.0, [0.0, y, 0.0], cloud)
        assert valid
        np.testing.assert_allclose(r, [expected], atol=1e-3)
        np.testing.assert_allclose(J[0], [0.0, -1.0, 0.0], atol=1e-3)
    for y in (0.4, -0.4):
        assert not sm.tsdf_match_residuals(grid, 1.0, [0.0, y, 0.0], cloud)[0]
    empty = _host(sm, mk.grid_of(golden, insert_golden, "ref_empty"))
    assert not sm.tsdf_match_residuals(empty, 1.0, [0.0, 0.0, 0.0],
                                       np.zeros((1, 3), np.float32))[0]


def _assert_close(pose, summary, golden, key):
    ref_pose, s = golden[key + "/pose"], golden[key + "/summary"]
    np.testing.assert_allclose([pose.x, pose.y, pose.theta], ref_pose, rtol=0, atol=1e-6)
    assert abs(summary["initial_cost"] - s[0]) <= 1e-9 * max(1.0, s[0])
    assert abs(summary["final_cost"] - s[1]) <= 1e-7 * max(1.0, s[1])
    assert summary["termination"] == int(s[4])
    assert summary["num_successful_steps"] == int(s[2])
    assert summary["num_unsuccessful_steps"] == int(s[3])


def _matcher(sm, golden, key):
    o = golden[key + "/options"]
    return sm.CeresScanMatcher2D(o[0], o[1], o[2], bool(o[3]), int(o[4]))


@pytest.mark.parametrize("case", _solve_cases())
def test_solves_match_the_reference_host_and_resident(sm, golden, insert_golden, case):
    key = f"solve/{case}"
    grid = mk.grid_of(golden, insert_golden, str(golden[key + "/grid"]))
    cloud = mk.cloud_of(golden, insert_golden, key)
    init = sm.Rigid2d(*golden[key + "/init"])
    target = golden[key + "/target"]
    m = _matcher(sm, golden, key)
    pose, summary = m.match(target, init, cloud, _host(sm, grid))
    _assert_close(pose, summary, golden, key)
    dev = _device(grid)
    pose_d, summary_d = m.match(target, init, cloud, dev)
    assert (pose_d.x, pose_d.y, pose_d.theta) == (pose.x, pose.y, pose.theta)
    assert summary_d == summary


def test_failure_and_failed_candidates_are_covered(golden):
    """The golden holds a FAILURE solve and solves whose candidates leave the known patch."""
    assert golden["solve/failure/summary"][4] == 2
    assert golden["solve/empty_cloud/summary"][4] == 2
    assert max(golden[f"solve/patch_{k}/summary"][3] for k in range(3)) > 0


def test_batch_is_bit_identical_and_passes_through(sm, golden, insert_golden):
    """refine_batch_tsdf on room solves (target = the pose's translation) equals per-problem
    resident and host-plane solves bit for bit; found == 0 entries come back unchanged."""
    grid = mk.grid_of(golden, insert_golden, "room")
    cloud = insert_golden["room_lua/3/returns"]
    dev = _device(grid)
    m = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, True, 10)
    rng = np.random.default_rng(5)
    poses = [sm.Rigid2d(*rng.uniform(-0.05, 0.05, 3)) for _ in range(6)]
    found = np.array([1, 1, 0, 1, 0, 1], np.int32)
    out, sums = m.refine_batch_tsdf([dev] * 6, found, poses, cloud)
    for k, p in enumerate(poses):
        if not found[k]:
            assert (out[k].x, out[k].y, out[k].theta) == (p.x, p.y, p.theta)
            assert sums[k]["termination"] == 1
            continue
        one, s1 = m.match([p.x, p.y], p, cloud, dev)
        host, s2 = m.match([p.x, p.y], p, cloud, _host(sm, grid))
        assert (out[k].x, out[k].y, out[k].theta) == (one.x, one.y, one.theta) == \
            (host.x, host.y, host.theta)
        assert sums[k] == s1 == s2


def test_batch_groups_grids_by_device(sm, golden, insert_golden):
    from cartographer_amd import _lib
    if _lib.lib().cmx_device_count() < 2:
        pytest.skip("one device")
    grid = mk.grid_of(golden, insert_golden, "room")
    cloud = insert_golden["room_lua/5/returns"]
    grids = [_device(grid, 0), _device(grid, 1), _device(grid, 0)]
    m = sm.CeresScanMatcher2D(1.0, 10.0, 40.0, False, 20)
    poses = [sm.Rigid2d(0.01 * k, -0.02, 0.01) for k in range(3)]
    out, sums = m.refine_batch_tsdf(grids, None, poses, cloud)
    for k, p in enumerate(poses):
        one, s1 = m.match([p.x, p.y], p, cloud, grids[k])
        assert (out[k].x, out[k].y, out[k].theta) == (one.x, one.y, one.theta)
        assert sums[k] == s1


def test_probability_grid_refinement_is_unchanged(sm, synth):
    """The probability-grid instance of the templated kernel: CeresScanMatcherTest's fixture
    (ceres_scan_matcher_2d_test.cc:34-112) still converges."""
    g = synth.ProbabilityGrid(1.0, (10.0, 10.0), 20, 20)
    g.set_probability(7, 13, 0.9)
    lim = g.limits
    cloud = np.array([[-3.0, 2.0, 0.0]], np.float32)
    m = sm.CeresScanMatcher2D(1.0, 0.1, 1.5, True, 50)
    pose, summary = m.match((-0.3, 0.5), sm.Rigid2d(-0.3, 0.5, 0.0), cloud,
                            sm.Grid2D(g.cells, 1.0, lim["max_x"], lim["max_y"]))
    assert abs(summary["final_cost"]) < 1e-2
    assert abs(pose.x + 0.5) < 1e-2 and abs(pose.y - 0.5) < 1e-2
