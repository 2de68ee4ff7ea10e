"""cmx_fast3d_match_pairs / cmx_fast3d_refine_pairs: many nodes against submaps in one fast-3D
batch (the burst of PoseGraph3D::ComputeConstraintsForNode when a submap finishes,
mapping/internal/3d/pose_graph_3d.cc:370-379).  Every pair must return bit for bit what the
single-pair calls return, which the rest of the suite pins to the oracle."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_3d import _assert_same_results, _fast3d_batch_scene
from test_oracle_reference_pins_3d import quat_from_angle_axis

pytestmark = pytest.mark.gpu

# High-resolution point counts around the wave (64) and block (256) boundaries of the discretise
# and scoring kernels, low-resolution counts from 77 down to 1.
HIGH_COUNTS = (384, 383, 129, 65, 64, 63, 2, 1)
LOW_COUNTS = (77, 60, 26, 13, 9, 5, 2, 1)


@pytest.fixture(scope="module")
def sm3():
    from cartographer_amd import _lib, scan_matching_3d
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching_3d


def _submap_histogram():
    k = np.arange(16, dtype=np.float64)
    return (np.exp(-((k - 5.0) / 1.5) ** 2) + 0.6 * np.exp(-((k - 12.0) / 1.0) ** 2) +
            0.05).astype(np.float32)


def _old_nodes_scene(sm3, synth):
    """One matcher with a peaked histogram and a yaw pre-filter that bites, eight nodes of their
    own: scans from different positions, cut to HIGH_COUNTS / LOW_COUNTS points, each with its
    own gravity alignment and its own histogram (the submap's, shifted and perturbed)."""
    submap_hist = _submap_histogram()
    opt = dict(branch_and_bound_depth=4, full_resolution_depth=2, min_rotational_score=0.8,
               min_low_resolution_score=0.2, linear_xy_search_window=1.0,
               linear_z_search_window=0.4, angular_search_window=math.radians(10.0))
    grid, world = synth.make_submap_3d(70, 0.2, (8.0, 8.0, 3.0), 4, 8, 96)
    vox = grid.voxels()
    matcher = sm3.FastCorrelativeScanMatcher3D(0.2, vox, grid.grid_size, 0.2, vox, submap_hist,
                                               **opt)
    rng = np.random.default_rng(17)
    datas, poses = [], []
    for k, (n_hi, n_lo) in enumerate(zip(HIGH_COUNTS, LOW_COUNTS)):
        pos = world.free_position(200 + k, 0.6)
        scan = world.scan(pos, 0.0, 7, 64, seed=k)
        assert scan.shape[0] >= 384
        hist = (np.roll(submap_hist, k % 3 - 1) *
                rng.uniform(0.8, 1.2, 16).astype(np.float32)).astype(np.float32)
        axis = [[1, 0, 0], [0, 1, 0], [1, 1, 0]][k % 3]
        datas.append(sm3.TrajectoryNodeData(scan[:n_hi].copy(), scan[::5][:n_lo].copy(), hist,
                                            tuple(quat_from_angle_axis(0.01 * (k + 1), axis))))
        d = rng.uniform(-0.3, 0.3, 3) * np.array([1.0, 1.0, 0.3])
        poses.append(sm3.Rigid3d(tuple(pos + d),
                                 tuple(quat_from_angle_axis(rng.uniform(-0.1, 0.1), [0, 0, 1]))))
    return matcher, datas, poses


@pytest.fixture(scope="module")
def old_nodes(sm3, synth):
    """The scene of _old_nodes_scene with the single calls' results and scan counts."""
    matcher, datas, poses = _old_nodes_scene(sm3, synth)
    ident = sm3.Rigid3d()
    expected, scans = [], []
    for data, pose in zip(datas, poses):
        expected.append(matcher.match(pose, ident, data, 0.12))
        scans.append(matcher.last_stats["num_scans"])
    return dict(matcher=matcher, datas=datas, poses=poses, expected=expected, scans=scans)


@pytest.fixture(scope="module")
def cross(sm3, synth):
    """Three nodes x four matchers of depths 3 to 6, windowed and full-submap pairs mixed, with
    the single calls' results."""
    matchers, pos, data0 = _fast3d_batch_scene(sm3, synth, [5, 4, 6, 3])
    hist = np.zeros(16, np.float32)
    _, world = synth.make_submap_3d(70, 0.2, (8.0, 8.0, 3.0), 4, 8, 96)
    datas, centres = [data0], [pos]
    for k in (1, 2):
        p = world.free_position(200 + k, 0.6)
        hi = world.scan(p, 0.0, 6, 64, seed=k)[:384 - 37 * k]
        datas.append(sm3.TrajectoryNodeData(hi, hi[::5].copy(), hist,
                                            tuple(quat_from_angle_axis(0.01 * (k + 1), [0, 1, 0]))))
        centres.append(p)
    rng = np.random.default_rng(5)
    pair_matchers, pair_datas, nodes, fulls, thresholds = [], [], [], [], []
    for k in range(12):
        node = k // 4
        d = rng.uniform(-0.3, 0.3, 3) * np.array([1.0, 1.0, 0.3])
        nodes.append(sm3.Rigid3d(tuple(centres[node] + d),
                                 tuple(quat_from_angle_axis(rng.uniform(-0.1, 0.1), [0, 0, 1]))))
        pair_matchers.append(matchers[k % 4])
        pair_datas.append(datas[node])
        fulls.append(k % 5 == 3)
        thresholds.append([0.12, 0.3, 0.99][k % 3] if k % 4 else 0.12)
    ident = sm3.Rigid3d()
    expected = [m.match_full_submap(node.rotation, ident.rotation, data, t) if full
                else m.match(node, ident, data, t)
                for m, node, full, t, data in zip(pair_matchers, nodes, fulls, thresholds,
                                                  pair_datas)]
    return dict(matchers=pair_matchers, datas=pair_datas, nodes=nodes, fulls=fulls,
                thresholds=thresholds, expected=expected)


def _match_cross(sm3, cross, datas=None):
    num = len(cross["matchers"])
    return sm3.fast3d_match_pairs(cross["matchers"], cross["nodes"], [sm3.Rigid3d()] * num,
                                  cross["fulls"], cross["thresholds"],
                                  cross["datas"] if datas is None else datas)


def test_old_nodes_against_one_submap(sm3, old_nodes):
    """Eight nodes of 384 ... 1 points against one matcher: clouds, histogram, gravity alignment
    and pose per pair, and a yaw pre-filter that keeps another set of scans for each."""
    scans, expected = old_nodes["scans"], old_nodes["expected"]
    assert len(set(scans)) > 1 and max(scans) > 0, scans
    assert any(e is not None for e in expected), "the parity check needs a found pair"
    num = len(old_nodes["datas"])
    got, stats = sm3.fast3d_match_pairs([old_nodes["matcher"]] * num, old_nodes["poses"],
                                        [sm3.Rigid3d()] * num, [False] * num, [0.12] * num,
                                        old_nodes["datas"])
    _assert_same_results(old_nodes["expected"], got)
    assert stats["num_scans"] == sum(scans)
    # pairs of unlike clouds share the expansion counters: lookups are not reported
    assert stats["expansion_lookups"] == 0


def test_cross_product_of_nodes_and_matchers(sm3, cross):
    expected = cross["expected"]
    assert any(e is not None for e in expected) and any(e is None for e in expected)
    got, stats = _match_cross(sm3, cross)
    _assert_same_results(expected, got)
    assert stats["num_scans"] > 0


def test_shared_pointers_equal_copies(sm3, cross):
    """Pairs that name one TrajectoryNodeData object (one upload) against pairs that name equal
    copies of it (an upload each)."""
    copies = [sm3.TrajectoryNodeData(d.high_resolution_point_cloud.copy(),
                                     d.low_resolution_point_cloud.copy(),
                                     d.rotational_scan_matcher_histogram.copy(),
                                     d.gravity_alignment) for d in cross["datas"]]
    assert len({id(d) for d in cross["datas"]}) == 3 and len({id(d) for d in copies}) == 12
    shared, _ = _match_cross(sm3, cross)
    separate, _ = _match_cross(sm3, cross, copies)
    _assert_same_results(shared, separate)
    _assert_same_results(cross["expected"], separate)


def test_shared_list_overflow_repeats_every_pair_alone(sm3, cross, debug):
    _, roomy = _match_cross(sm3, cross)
    debug(frontier_capacity=4096)
    got, cramped = _match_cross(sm3, cross)
    _assert_same_results(cross["expected"], got)
    # the repeated searches' candidates are added to the shared chain's
    assert cramped["candidates_scored"] > roomy["candidates_scored"]


def test_depth_one_matcher_takes_the_fallback(sm3, synth, cross):
    matchers, _, _ = _fast3d_batch_scene(sm3, synth, [1, 4])
    ident = sm3.Rigid3d()
    pair_matchers = [matchers[0], matchers[1], matchers[0], matchers[1]]
    datas = [cross["datas"][0], cross["datas"][4], cross["datas"][8], cross["datas"][0]]
    nodes = [cross["nodes"][0], cross["nodes"][4], cross["nodes"][8], cross["nodes"][1]]
    expected = [m.match(node, ident, data, 0.12)
                for m, node, data in zip(pair_matchers, nodes, datas)]
    got, _ = sm3.fast3d_match_pairs(pair_matchers, nodes, [ident] * 4, [False] * 4, [0.12] * 4,
                                    datas)
    _assert_same_results(expected, got)


def test_chunked_batch_equals_the_unsplit_one(sm3, old_nodes, debug):
    """fast3d_chunk_cells caps the rotated points (scans x points, summed) of a chain of
    launches: the eight pairs then run as consecutive sub-batches."""
    num = len(old_nodes["datas"])
    args = ([old_nodes["matcher"]] * num, old_nodes["poses"], [sm3.Rigid3d()] * num,
            [False] * num, [0.12] * num, old_nodes["datas"])
    _, unsplit = sm3.fast3d_match_pairs(*args)
    cells = [s * n for s, n in zip(old_nodes["scans"], HIGH_COUNTS)]
    cap = max(cells) + 1
    # the planner's rule: a sub-batch takes consecutive pairs while its cells stay below the cap
    chunks, pairs, total = 1, 0, 0
    for c in cells:
        if pairs and total + c >= cap:
            chunks, pairs, total = chunks + 1, 0, 0
        pairs, total = pairs + 1, total + c
    assert chunks >= 3, (cells, cap)
    debug(fast3d_chunk_cells=cap)
    got, split = sm3.fast3d_match_pairs(*args)
    _assert_same_results(old_nodes["expected"], got)
    assert split["num_scans"] == unsplit["num_scans"]
    # one matcher: every chain of launches expands the same number of levels
    assert unsplit["expansion_launches"] > 0
    assert split["expansion_launches"] >= 3 * unsplit["expansion_launches"]


def test_refine_pairs_equals_refine_batch_pair_by_pair(sm3, cross):
    ceres = sm3.CeresScanMatcher3D([5.0, 20.0], 10.0, 1.0, only_optimize_yaw=False,
                                   use_nonmonotonic_steps=False, max_num_iterations=10)
    results, _ = _match_cross(sm3, cross)
    found = [r is not None for r in results]
    assert any(found) and not all(found)
    passed = sm3.Rigid3d((0.5, -0.25, 0.125), tuple(quat_from_angle_axis(0.3, [0, 0, 1])))
    poses = [r["pose_estimate"] if r is not None else passed for r in results]
    refined, summaries = ceres.refine_pairs(cross["matchers"], found, poses, cross["datas"])
    for k, (m, f, pose, data) in enumerate(zip(cross["matchers"], found, poses, cross["datas"])):
        single, summary = ceres.refine_batch([m], [f], [pose], data)
        assert refined[k] == single[0], (k, refined[k], single[0])
        assert summaries[k] == summary[0], (k, summaries[k], summary[0])
        if not f:
            assert refined[k] == passed and summaries[k]["num_successful_steps"] == 0


def _raw_match_pairs(sm3, matchers, pointers, num_pairs):
    """cmx_fast3d_match_pairs with identity poses, windowed, for the argument checks: returns
    (status, last error)."""
    from cartographer_amd import _lib
    L = _lib.lib()
    n = max(len(matchers), 1)
    handles = (C.c_void_p * n)(*[m._h for m in matchers])
    poses = (_lib.Pose3d * n)(*[sm3.Rigid3d().to_c() for _ in range(n)])
    full = np.zeros(n, np.int32)
    thresholds = np.full(n, 0.12, np.float32)
    found = np.zeros(n, np.int32)
    results = (_lib.Result3D * n)()
    stats = _lib.MatchStats()
    status = L.cmx_fast3d_match_pairs(handles, num_pairs, C.cast(poses, C.c_void_p),
                                      C.cast(poses, C.c_void_p), full.ctypes.data,
                                      thresholds.ctypes.data, pointers, found.ctypes.data,
                                      C.cast(results, C.c_void_p), C.byref(stats))
    return status, L.cmx_last_error().decode()


def test_invalid_arguments(sm3, cross):
    from cartographer_amd import _lib
    matchers = cross["matchers"][:2]
    good = cross["datas"][0].to_c()
    pointer_type = C.POINTER(_lib.NodeData3D)
    # a null entry in data
    status, error = _raw_match_pairs(sm3, matchers,
                                     (pointer_type * 2)(C.pointer(good), pointer_type()), 2)
    assert status == _lib.INVALID_ARGUMENT and "null" in error
    # a histogram of another size than its matcher's (16 bins)
    d = cross["datas"][0]
    short = sm3.TrajectoryNodeData(d.high_resolution_point_cloud, d.low_resolution_point_cloud,
                                   np.zeros(8, np.float32), d.gravity_alignment).to_c()
    status, error = _raw_match_pairs(sm3, matchers,
                                     (pointer_type * 2)(C.pointer(good), C.pointer(short)), 2)
    assert status == _lib.INVALID_ARGUMENT and "histogram" in error
    # no pairs
    status, error = _raw_match_pairs(sm3, matchers,
                                     (pointer_type * 2)(C.pointer(good), C.pointer(good)), 0)
    assert status == _lib.INVALID_ARGUMENT and "num_pairs" in error
    # the same through cmx_fast3d_refine_pairs
    L = _lib.lib()
    ceres = sm3.CeresScanMatcher3D([5.0, 20.0], 10.0, 1.0)
    handles = (C.c_void_p * 2)(*[m._h for m in matchers])
    poses = (_lib.Pose3d * 2)(sm3.Rigid3d().to_c(), sm3.Rigid3d().to_c())
    out = (_lib.Pose3d * 2)()
    for pointers, num_pairs, word in (
            ((pointer_type * 2)(C.pointer(good), pointer_type()), 2, "null"),
            ((pointer_type * 2)(C.pointer(good), C.pointer(good)), 0, "num_pairs")):
        status = L.cmx_fast3d_refine_pairs(C.byref(ceres.options), handles, num_pairs, None,
                                           C.cast(poses, C.c_void_p), pointers,
                                           C.cast(out, C.c_void_p), None)
        assert status == _lib.INVALID_ARGUMENT and word in L.cmx_last_error().decode()


def test_matchers_on_different_devices_are_refused(sm3, synth, cross):
    from cartographer_amd import _lib
    if _lib.lib().cmx_device_count() < 2:
        pytest.skip("needs two devices")
    grid, _ = synth.make_submap_3d(70, 0.2, (8.0, 8.0, 3.0), 4, 8, 96)
    vox = grid.voxels()
    other = sm3.FastCorrelativeScanMatcher3D(0.2, vox, grid.grid_size, 0.2, vox,
                                             np.zeros(16, np.float32), branch_and_bound_depth=4,
                                             full_resolution_depth=2, device=1)
    good = cross["datas"][0].to_c()
    pointers = (C.POINTER(_lib.NodeData3D) * 2)(C.pointer(good), C.pointer(good))
    status, error = _raw_match_pairs(sm3, [cross["matchers"][0], other], pointers, 2)
    assert status == _lib.INVALID_ARGUMENT and "device" in error


def test_constraint_builder_flushes_all_nodes_in_one_call(sm3, synth):
    """Two nodes x three submaps queued before when_done: the constraints of the per-pair calls
    (search, then refinement), in the order the pairs were added."""
    from cartographer_amd import constraint_builder as cb
    hist = np.zeros(16, np.float32)
    options = cb.ConstraintBuilderOptions3D(
        sampling_ratio=1.0, max_constraint_distance=50.0, min_score=0.12,
        global_localization_min_score=0.12, branch_and_bound_depth=4, full_resolution_depth=2,
        min_rotational_score=0.0, min_low_resolution_score=0.1, linear_xy_search_window=0.6,
        linear_z_search_window=0.2, angular_search_window=math.radians(5.0))
    submaps, world = [], None
    for seed in (70, 71, 72):
        grid, w = synth.make_submap_3d(seed, 0.2, (8.0, 8.0, 3.0), 4, 8, 96)
        world = world or w
        submaps.append(cb.Submap3D(0.2, grid.voxels(), grid.grid_size, 0.2, grid.voxels(), hist))
    nodes = []
    for k in range(2):
        pos = world.free_position(200 + k, 0.6)
        hi = world.scan(pos, 0.0, 6, 64, seed=k)[:384 - 50 * k]
        data = sm3.TrajectoryNodeData(hi, hi[::5].copy(), hist,
                                      tuple(quat_from_angle_axis(0.01 * (k + 1), [1, 0, 0])))
        pose = sm3.Rigid3d(tuple(pos + np.array([0.1, -0.1, 0.05]) * (k + 1)),
                           tuple(quat_from_angle_axis(0.03 * k, [0, 0, 1])))
        nodes.append((data, pose))
    ceres = sm3.CeresScanMatcher3D([5.0, 20.0], 10.0, 1.0, max_num_iterations=10)
    builder = cb.ConstraintBuilder3D(options, ceres=ceres)
    ident = sm3.Rigid3d()
    for j, (data, pose) in enumerate(nodes):
        for i, submap in enumerate(submaps):
            builder.maybe_add_constraint((0, i), submap, (0, j), data, pose, ident)
    out = []
    builder.when_done(out.extend)
    expected = []
    for j, (data, pose) in enumerate(nodes):
        for i in range(len(submaps)):
            matcher = builder._scan_matchers[(0, i)]
            result = matcher.match(pose, ident, data, options.min_score)
            if result is None:
                continue
            refined, _ = ceres.refine_batch([matcher], [True], [result["pose_estimate"]], data)
            expected.append(((0, i), (0, j), refined[0], result["score"]))
    assert len(expected) >= 2
    assert [(c.submap_id, c.node_id, c.zbar_ij, c.score) for c in out] == expected
