"""cmx_rt3d_match_grid_batch and cmx_ceres3d_match_grids_batch on the GPU: LocalTrajectoryBuilder3D
::ScanMatch's two matchers for many trajectories in one call each, bit for bit the single calls
(np.float32 score and all seven pose numbers), on one small world: four sweeps of 6 rings x 64 into
resident grids at 0.1 m and 0.2 m.

Windows.  The linear window of most tests is 0.2 m: two steps (125 translations) at 0.1 m and one
(27) at 0.2 m, neither a multiple of the 64 translations of a block.  The window of
trajectory_builder_3d.lua, 0.15 m, is ONE step at 0.1 m (the double 0.15 over the float 0.1f is
1.4999999776; tests/test_abi_rt3d_match_batch.py): 27 translations."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WINDOW = (0.2, math.radians(1.0))
LUA = (0.15, math.radians(1.0))


class _World:
    pass


def _sweep(world, p):
    pos = world.free_position(50 + p, 0.5)
    sensor = world.scan(pos, 0.2 * p, 6, 64, seed=p).astype(np.float64)
    c, s = math.cos(0.2 * p), math.sin(0.2 * p)
    in_map = np.stack([pos[0] + c * sensor[:, 0] - s * sensor[:, 1],
                       pos[1] + s * sensor[:, 0] + c * sensor[:, 1],
                       pos[2] + sensor[:, 2]], 1).astype(np.float32)
    return pos, in_map


@pytest.fixture(scope="module")
def scene(synth):
    """The grids of test_rt3d_on_the_device_built_grid at two resolutions, a scan cut to the sizes
    around a chunk of 64 points, and poses near the last sweep's."""
    from cartographer_amd import grid_3d, scan_matching_3d as sm3
    from test_oracle_reference_pins_3d import quat_from_angle_axis
    w = _World()
    w.world = synth.World3D(5, (8.0, 8.0, 4.0))
    w.hi, w.lo = grid_3d.HybridGridOnDevice(0.1), grid_3d.HybridGridOnDevice(0.2)
    for p in range(4):
        pos, in_map = _sweep(w.world, p)
        for g in (w.hi, w.lo):
            g.insert(pos.astype(np.float32), in_map, 0.7, 0.4, 2)
    w.pos = pos
    cloud = np.ascontiguousarray(w.world.scan(pos, 0.6, 6, 64, seed=9), np.float32)
    assert cloud.shape == (384, 3)
    # (copies: equal pointers are one cloud to the call)
    w.clouds = {n: cloud[:n].copy() for n in (1, 63, 64, 65, 200, 384)}

    def pose(dx, dy, dz, yaw, axis=(0, 0, 1)):
        return sm3.Rigid3d(tuple(pos + np.array([dx, dy, dz])),
                           tuple(quat_from_angle_axis(yaw, list(axis))))
    w.pose = pose
    return w


def _numbers(score, pose):
    return [np.float32(score)] + list(pose.translation) + list(pose.rotation)


def _singles(matcher, poses, clouds, grids):
    return [_numbers(*matcher.match_grid(p, c, g)) for p, c, g in zip(poses, clouds, grids)]


def _batch(matcher, poses, clouds, grids):
    scores, out, stats = matcher.match_grid_batch(poses, clouds, grids)
    assert scores.dtype == np.float32
    return [_numbers(s, p) for s, p in zip(scores, out)], stats


def _mixed(scene):
    """Seven matches: the six cloud sizes, both grids (125 and 27 translations in one launch), the
    0.1 m grid in four of them, the 200-point cloud by one pointer in two, poses all different."""
    c = scene.clouds
    clouds = [c[1], c[63], c[64], c[65], c[200], c[384], c[200]]
    grids = [scene.hi, scene.lo, scene.hi, scene.lo, scene.hi, scene.lo, scene.lo]
    poses = [scene.pose(0.07, -0.04, 0.02, 0.61), scene.pose(-0.05, 0.03, 0.0, 0.58),
             scene.pose(0.0, 0.0, 0.0, 0.6), scene.pose(0.11, 0.02, -0.03, 0.63, (0.02, -0.01, 1)),
             scene.pose(-0.02, -0.09, 0.04, 0.59), scene.pose(0.04, 0.04, 0.01, 0.62),
             scene.pose(0.01, -0.01, 0.0, 0.6, (0.01, 0.03, 1))]
    return poses, clouds, grids


def _norms(clouds):
    return [float(np.sqrt((np.asarray(c, np.float64) ** 2).sum(1)).max()) for c in clouds]


def test_mixed_batch_equals_the_single_calls_and_the_oracle(scene, oracle):
    from cartographer_amd import scan_matching_3d as sm3
    m = sm3.RealTimeCorrelativeScanMatcher3D(*WINDOW, 0.1, 0.1)
    poses, clouds, grids = _mixed(scene)
    plan = sm3.rt3d_batch_plan(m, [g.resolution for g in grids], [len(c) for c in clouds],
                               _norms(clouds))
    assert {p["T"] for p in plan} == {125, 27}
    assert [p["set"] for p in plan] == [0] * 7                    # one launch set
    got, stats = _batch(m, poses, clouds, grids)
    assert got == _singles(m, poses, clouds, grids)
    assert stats["candidates_scored"] == sum(p["T"] * p["R"] for p in plan)
    assert stats["num_scans"] == sum(p["R"] for p in plan)
    for k in (4, 5):
        init = list(poses[k].translation) + list(poses[k].rotation)
        ref = oracle.rt3d_match(grids[k].resolution, grids[k].voxels(), init, clouds[k], WINDOW[0],
                                WINDOW[1], 0.1, 0.1)
        assert got[k][0] == np.float32(ref["score"])
        np.testing.assert_array_equal(got[k][1:], ref["pose"])


def test_every_route_gives_the_same_result(scene, debug):
    from cartographer_amd import scan_matching_3d as sm3
    m = sm3.RealTimeCorrelativeScanMatcher3D(*WINDOW, 0.1, 0.1)
    poses, clouds, grids = _mixed(scene)
    plan = sm3.rt3d_batch_plan(m, [g.resolution for g in grids], [len(c) for c in clouds],
                               _norms(clouds))
    assert [p["route"] for p in plan] == [0] * 7                  # by size: all segmented
    by_size, _ = _batch(m, poses, clouds, grids)
    debug(rt3d_batch_route=1)
    segmented, _ = _batch(m, poses, clouds, grids)
    debug(rt3d_batch_route=2)
    single, stats = _batch(m, poses, clouds, grids)
    assert by_size == segmented == single
    assert stats["candidates_scored"] == sum(p["T"] * p["R"] for p in plan)


def test_points_far_outside_the_brick(scene):
    """Points beyond every face of the brick and candidates that put even the near ones outside:
    every lookup outside the brick reads kMinProbability, as the padded brick's border does."""
    from cartographer_amd import scan_matching_3d as sm3
    m = sm3.RealTimeCorrelativeScanMatcher3D(*WINDOW, 0.1, 0.1)
    far = np.array([[30, 0, 0], [-30, 0, 0], [0, 30, 0], [0, -30, 0], [0, 0, 30], [0, 0, -30],
                    [25, 25, 25], [-25, -25, -25], [0.5, 0.5, 0.2], [1.5, -0.5, 0.1]], np.float32)
    mixed = np.ascontiguousarray(np.concatenate([scene.clouds[65], far]))
    away = sm3.Rigid3d((100.0, -100.0, 50.0), scene.pose(0, 0, 0, 0.3).rotation)
    poses = [scene.pose(0.02, 0.01, 0.0, 0.6), away, away, scene.pose(0.0, 0.03, 0.0, 0.61)]
    clouds = [mixed, scene.clouds[65], far, far]
    grids = [scene.hi, scene.hi, scene.lo, scene.lo]
    got, _ = _batch(m, poses, clouds, grids)
    assert got == _singles(m, poses, clouds, grids)
    assert got[1][0] < np.float32(0.11)                  # nothing but kMinProbability out there


def test_single_candidate_windows_next_to_a_normal_match(scene):
    """0.1 m is no step at 0.2 m (0.49999999 rounds to 0) and one at 0.1 m; a cloud within 0.6 m
    has an angular step of 19 degrees: L = 0 and A = 0, one candidate, one block."""
    from cartographer_amd import scan_matching_3d as sm3
    m = sm3.RealTimeCorrelativeScanMatcher3D(0.1, math.radians(1.0), 0.1, 0.1)
    tiny = np.ascontiguousarray(scene.clouds[65] * np.float32(0.02))
    poses = [scene.pose(0.0, 0.0, 0.0, 0.6), scene.pose(0.03, 0.0, 0.01, 0.6),
             scene.pose(0.0, 0.02, 0.0, 0.6)]
    clouds, grids = [tiny, scene.clouds[200], tiny], [scene.lo, scene.hi, scene.lo]
    plan = sm3.rt3d_batch_plan(m, [g.resolution for g in grids], [len(c) for c in clouds],
                               _norms(clouds))
    assert [(p["T"], p["R"], p["blocks"]) for p in plan][::2] == [(1, 1, 1)] * 2
    assert plan[1]["T"] == 27 and plan[1]["R"] > 1
    got, stats = _batch(m, poses, clouds, grids)
    assert got == _singles(m, poses, clouds, grids)
    assert stats["candidates_scored"] == 2 + plan[1]["T"] * plan[1]["R"]


def test_flat_landscape_takes_the_rerun(scene, oracle):
    """An empty grid and zero weights at the lua window: every candidate (27 translations times the
    rotations this small world's range gives) scores kMinProbability, the finalist list overflows
    and the match runs again through the single path; the first candidate wins.  The normal match
    of the call is not affected."""
    from cartographer_amd import grid_3d, scan_matching_3d as sm3
    m = sm3.RealTimeCorrelativeScanMatcher3D(*LUA, 0.0, 0.0)
    empty = grid_3d.HybridGridOnDevice(0.1)
    poses = [scene.pose(0.07, -0.04, 0.02, 0.61), scene.pose(0.0, 0.01, 0.0, 0.6)]
    clouds, grids = [scene.clouds[200], scene.clouds[200]], [empty, scene.hi]
    plan = sm3.rt3d_batch_plan(m, [0.1, 0.1], [200, 200], _norms(clouds))
    candidates = plan[0]["T"] * plan[0]["R"]
    assert plan[0]["T"] == 27 and candidates > 128 and plan[0]["route"] == 0   # (a list holds 128)
    got, stats = _batch(m, poses, clouds, grids)
    assert got == _singles(m, poses, clouds, grids)
    init = list(poses[0].translation) + list(poses[0].rotation)
    ref = oracle.rt3d_match(0.1, scene.hi.voxels()[:0], init, clouds[0], LUA[0], LUA[1], 0.0, 0.0)
    assert got[0][0] == np.float32(ref["score"]) and abs(got[0][0] - 0.1) < 1e-6
    np.testing.assert_array_equal(got[0][1:], ref["pose"])
    assert stats["candidates_scored"] == 2 * candidates


def test_an_insertion_between_two_calls_is_seen(synth):
    """Nothing derived from a grid outlives a call: grids of this test's own, so that the module's
    scene stays as it is."""
    from cartographer_amd import grid_3d, scan_matching_3d as sm3
    from test_oracle_reference_pins_3d import quat_from_angle_axis
    world = synth.World3D(5, (8.0, 8.0, 4.0))
    grids = [grid_3d.HybridGridOnDevice(0.1), grid_3d.HybridGridOnDevice(0.2)]
    sweeps = [_sweep(world, p) for p in range(4)]
    for pos, in_map in sweeps[:2]:
        for g in grids:
            g.insert(pos.astype(np.float32), in_map, 0.7, 0.4, 2)
    pos = sweeps[3][0]
    cloud = np.ascontiguousarray(world.scan(pos, 0.6, 6, 64, seed=9)[:200], np.float32)
    m = sm3.RealTimeCorrelativeScanMatcher3D(*WINDOW, 0.1, 0.1)
    poses = [sm3.Rigid3d(tuple(pos + np.array([0.05, 0.0, 0.0])),
                         tuple(quat_from_angle_axis(0.6, [0, 0, 1])))] * 2
    before, _ = _batch(m, poses, [cloud, cloud], grids)
    assert before == _singles(m, poses, [cloud, cloud], grids)
    for pos, in_map in sweeps[2:]:
        grids[0].insert(pos.astype(np.float32), in_map, 0.7, 0.4, 2)
    after, _ = _batch(m, poses, [cloud, cloud], grids)
    assert after == _singles(m, poses, [cloud, cloud], grids)
    assert after[0] != before[0] and after[1] == before[1]       # only the first grid changed


def test_a_bad_match_in_the_middle_leaves_the_outputs_alone(scene):
    from cartographer_amd import _lib
    poses, clouds, grids = _mixed(scene)
    num = len(grids)
    options = _lib.RtOptions(WINDOW[0], WINDOW[1], 0.1, 0.1)
    handles = (C.c_void_p * num)(*[g._h for g in grids])
    pointers = (C.c_void_p * num)(*[c.ctypes.data for c in clouds])
    inits = (_lib.Pose3d * num)(*[p.to_c() for p in poses])
    scores = np.full(num, -7.0, np.float32)
    out = (_lib.Pose3d * num)()
    for p in out:
        p.t[0] = -7.0
    for counts, word in [([1, 63, 64, 0, 200, 384, 200], "match 3"),
                         ([1, 63, 64, 65, 200, 384, 199], "match 6")]:
        counts = np.array(counts, np.int32)
        status = _lib.lib().cmx_rt3d_match_grid_batch(
            C.byref(options), handles, num, C.cast(inits, C.c_void_p), pointers,
            counts.ctypes.data, scores.ctypes.data, C.cast(out, C.c_void_p), None)
        assert status == _lib.INVALID_ARGUMENT
        assert word in _lib.lib().cmx_last_error().decode()
        assert np.all(scores == -7.0) and all(p.t[0] == -7.0 for p in out)


def test_ceres_batch_equals_the_single_calls_and_the_oracle(scene, oracle):
    """Three robots, two pairs each: clouds of 1, 65 and 200 points, the 200- and 65-point clouds
    by one pointer in two robots, an empty low-resolution grid in the second, targets away from the
    initial translations (what a real-time match leaves)."""
    from cartographer_amd import grid_3d, scan_matching_3d as sm3
    c = scene.clouds
    empty = grid_3d.HybridGridOnDevice(0.2)
    pairs = [[(c[200], scene.hi), (c[65], scene.lo)],
             [(c[65], scene.hi), (c[1], empty)],
             [(c[200], scene.hi), (c[65], scene.lo)]]
    poses = [scene.pose(0.03, -0.02, 0.01, 0.61, (0.02, -0.01, 1.0)),
             scene.pose(-0.02, 0.01, 0.0, 0.59), scene.pose(0.01, 0.03, -0.01, 0.6)]
    targets = [np.array(p.translation) + d for p, d in
               zip(poses, ([0.02, 0.0, -0.01], [-0.01, 0.02, 0.0], [0.0, -0.03, 0.01]))]
    m = sm3.CeresScanMatcher3D([1.0, 6.0], 5.0, 4e2, max_num_iterations=12)
    got_poses, got_summaries = sm3.ceres_match_grids_batch(m, targets, poses, pairs)
    for k in range(3):
        pose, summary = m.match_grids(targets[k], poses[k], pairs[k])
        assert got_poses[k] == pose and got_summaries[k] == summary, k
    assert got_summaries[0]["num_successful_steps"] >= 1
    init = list(poses[0].translation) + list(poses[0].rotation)
    listed = [(c[200], 0.1, scene.hi.voxels()), (c[65], 0.2, scene.lo.voxels())]
    ref = oracle.ceres3d_match(listed, targets[0], init, [1.0, 6.0], translation_weight=5.0,
                               rotation_weight=4e2, max_num_iterations=12)
    np.testing.assert_allclose(list(got_poses[0].translation) + list(got_poses[0].rotation),
                               ref["pose"], rtol=0, atol=1e-6)
    assert got_summaries[0]["num_successful_steps"] == ref["num_successful_steps"]
    assert got_summaries[0]["num_unsuccessful_steps"] == ref["num_unsuccessful_steps"]
