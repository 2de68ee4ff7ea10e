"""cmx_grid3d_insert_batch on the device: range data into many resident hybrid grids in one call
must leave every grid -- grid_size and every voxel -- exactly as the same insertions made one by
one leave it.  Every comparison is made twice: against synth.HybridGrid (the host restatement of
the reference's inserter that tests/test_oracle_reference_pins_3d.py pins to the reference) and
against a second set of device grids filled by single cmx_grid3d_insert calls.  No downloaded
voxel may keep the update marker (bit 15)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# RangeDataInserter3DTest's fixture (mapping/3d/range_data_inserter_3d_test.cc:28-53).
FIXTURE_ORIGIN = np.array([0, 0, -4], np.float32)
FIXTURE_RETURNS = np.array([[-3, -1, 4], [-2, 0, 4], [-1, 1, 4], [0, 2, 4]], np.float32)


@pytest.fixture(scope="module")
def g3():
    from cartographer_amd import _lib, grid_3d
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return grid_3d


def _assert_same(batch, single, host, where=""):
    for k, (b, s, h) in enumerate(zip(batch, single, host)):
        voxels = b.voxels()
        assert not (voxels["value"] & 0x8000).any(), (where, k)
        assert b.grid_size == h.grid_size, (where, k)
        assert s.grid_size == h.grid_size, (where, k)
        np.testing.assert_array_equal(voxels, h.voxels(), err_msg=f"{where} grid {k}: host")
        np.testing.assert_array_equal(voxels, s.voxels(), err_msg=f"{where} grid {k}: single calls")


def _check(g3, synth, resolutions, insertions, hit=0.7, miss=0.4, free=5, calls=None):
    """`insertions` = (grid index, origin, returns).  One batch call (or one per slice of `calls`)
    into one set of device grids, single calls into a second set and into host grids, compared
    after every call; returns (batch grids, host grids)."""
    batch = [g3.HybridGridOnDevice(r) for r in resolutions]
    single = [g3.HybridGridOnDevice(r) for r in resolutions]
    host = [synth.HybridGrid(r) for r in resolutions]
    for part in calls or [slice(None)]:
        g3.insert_batch([(batch[g], o, r) for g, o, r in insertions[part]], hit, miss, free)
        for g, origin, returns in insertions[part]:
            single[g].insert(origin, returns, hit, miss, free)
            if len(returns):
                host[g].insert(origin, returns, hit, miss, free)
        _assert_same(batch, single, host, f"after {part}")
    return batch, host


def _value_at(grid, x, y, z):
    v = grid.voxels()
    hit = v[(v["x"] == x) & (v["y"] == y) & (v["z"] == z)]
    return int(hit["value"][0]) if len(hit) else 0


# ---- 1. the reference's own fixture ---------------------------------------------------------
def test_reference_fixture_through_a_batch_of_one_and_three_rounds_on_one_grid(g3, synth):
    """RangeDataInserter3DTest.InsertPointCloud (range_data_inserter_3d_test.cc:97-114) through a
    batch of one; then three more insertions of the fixture in ONE call: three rounds on one
    grid."""
    one = [(0, FIXTURE_ORIGIN, FIXTURE_RETURNS)]
    (dev,), _ = _check(g3, synth, [1.0], one, 0.7, 0.4, 1000)
    at = {(int(r["x"]), int(r["y"]), int(r["z"])): int(r["value"]) for r in dev.voxels()}
    assert (0, 0, -4) in at and (0, 0, -3) in at and (0, 0, -2) in at      # misses along a ray
    for x in range(-4, 5):
        for y in range(-4, 5):
            assert ((x, y, 4) in at) == (not (x < -3 or x > 0 or y != x + 2))   # the four hits
    assert at[(-2, 0, 4)] > at[(-2, 0, 3)]                                  # hit 0.7 > miss 0.4
    (dev,), (host,) = _check(g3, synth, [1.0], one * 4, 0.7, 0.4, 1000,
                             calls=[slice(0, 1), slice(1, 4)])
    assert _value_at(dev, -2, 0, 4) > at[(-2, 0, 4)]                         # it did progress


# ---- 2. the ActiveSubmaps3D shape -----------------------------------------------------------
@pytest.fixture(scope="module")
def scan(synth):
    """300 returns of a simulated room around the sensor, and the 257 nearest of them."""
    world = synth.World3D(4, (8.0, 8.0, 4.0))
    position = world.free_position(41, 0.5)
    cloud = world.scan(position, 0.3, 4, 96, seed=2)[:300].astype(np.float32)
    assert cloud.shape == (300, 3)
    near = cloud[np.argsort(np.linalg.norm(cloud, axis=1), kind="stable")[:257]].copy()
    return cloud, near


def _submap_step(scan, shift):
    """The four insertions of one ActiveSubmaps3D::InsertData: two submaps (the sensor at
    different places in their frames), a near cloud into the 0.1 m grid and the full cloud into
    the 0.45 m grid of each.  `shift` moves the sensor in the first submap's high-resolution grid
    only."""
    cloud, near = scan
    out = []
    for submap, at in enumerate([(1.0, -2.0, 0.5), (-3.5, 0.7, -0.2)]):
        origin = np.array(at, np.float32)
        moved = origin + np.array([shift if submap == 0 else 0, 0, 0], np.float32)
        out.append((2 * submap, moved, near + moved))
        out.append((2 * submap + 1, origin, cloud + origin))
    return out


def test_the_four_insertions_of_active_submaps_3d_in_one_call(g3, synth, scan):
    """Four distinct grids of two resolutions, all empty: all four grow.  In the second call the
    same clouds come again -- three bricks stay -- except that the first grid's cloud lies 5 m
    (50 voxels, more than the 16 a brick is padded to) further on: that one grows."""
    _check(g3, synth, [0.1, 0.45, 0.1, 0.45], _submap_step(scan, 0.0) + _submap_step(scan, 5.0),
           0.55, 0.49, 2, calls=[slice(0, 4), slice(4, 8)])


# ---- 3. a mixed round -----------------------------------------------------------------------
MIXED_RESOLUTIONS = [0.1, 0.1, 0.45, 0.2, 0.1]
# (grid, returns): round 0 is the insertions 0 .. 4 -- one return next to 257 next to 256, the
# smallest shape at which a wrong block table crosses insertions, then none at all, then the two
# rays that have fewer samples than free-space voxels.
MIXED_LIST = [(0, 1), (1, 257), (2, 256), (3, 0), (4, "short"), (1, 3), (0, 300), (3, 64),
              (1, 0), (0, 2)]


def _mixed():
    rng = np.random.default_rng(17)
    out = []
    for grid, returns in MIXED_LIST:
        origin = rng.uniform(-0.5, 0.5, 3).astype(np.float32)
        if returns == "short":
            # a hit in the origin's own voxel (num_samples == 0), and a ray of 2 voxels: with 5
            # free-space voxels the sample positions -3 .. -1 are skipped
            origin = np.array([0.02, 0.01, -0.03], np.float32)
            points = np.array([[0.03, 0.02, -0.02], [0.21, 0.01, -0.03]], np.float32)
        else:
            points = (origin + rng.uniform(-3.0, 3.0, (returns, 3))).astype(np.float32)
        out.append((grid, origin, points))
    return out


@pytest.mark.parametrize("free", [0, 1, 5])
def test_mixed_list_equals_the_single_calls(g3, synth, free):
    _check(g3, synth, MIXED_RESOLUTIONS, _mixed(), 0.7, 0.4, free)


# ---- 6. rounds cut into sets of launches ----------------------------------------------------
@pytest.mark.parametrize("chain", [1, 2])
def test_rounds_cut_into_sets_of_launches_give_the_same_voxels(g3, synth, debug, chain):
    """grid3d_insert_chain: the round of five insertions goes out as five (three) sets."""
    debug(grid3d_insert_chain=chain)
    _check(g3, synth, MIXED_RESOLUTIONS, _mixed())


# ---- 4. order across rounds -----------------------------------------------------------------
def test_a_later_insertions_miss_falls_on_an_earlier_ones_hit(g3, synth):
    """A hits voxel X = (3, 0, 0); B's ray to (6, 0, 0) passes a miss through X.  Three A first
    saturate X at the upper bound, where the order of the last two shows: hit (clamped, no change)
    then miss ends below the bound, miss then hit ends on it."""
    origin = np.zeros(3, np.float32)
    a = (0, origin, np.array([[3, 0, 0]], np.float32))
    b = (0, origin, np.array([[6, 0, 0]], np.float32))
    (hit_miss,), (host_hit_miss,) = _check(g3, synth, [1.0], [a, a, a, a, b])
    (miss_hit,), (host_miss_hit,) = _check(g3, synth, [1.0], [a, a, a, b, a])
    assert _value_at(host_hit_miss, 3, 0, 0) < _value_at(host_miss_hit, 3, 0, 0)
    assert _value_at(hit_miss, 3, 0, 0) == _value_at(host_hit_miss, 3, 0, 0)
    assert _value_at(miss_hit, 3, 0, 0) == _value_at(host_miss_hit, 3, 0, 0)


# ---- 5. one cloud object, two resolutions ---------------------------------------------------
def test_the_same_cloud_object_into_two_grids_of_different_resolution(g3, synth, scan):
    """One array object: one pointer in both insertions, one upload."""
    cloud, _ = scan
    origin = np.zeros(3, np.float32)
    _check(g3, synth, [0.1, 0.45], [(0, origin, cloud), (1, origin, cloud)], 0.55, 0.49, 2)


# ---- 7. grid_size doubling ------------------------------------------------------------------
def test_grid_size_doubles_in_the_second_round(g3, synth):
    """A return 6.45 m out at 0.1 m is voxel 65 (f32: 64.5, rounded away from zero): past the 63
    a grid_size of 128 holds."""
    origin = np.array([5.0, 0.0, 0.0], np.float32)
    first = (0, origin, np.array([[5.5, 0.2, 0.1], [4.0, -0.3, 0.0]], np.float32))
    second = (0, origin, np.array([[6.45, 0.0, 0.0]], np.float32))
    (dev,), (host,) = _check(g3, synth, [0.1], [first], free=2)
    assert dev.grid_size == host.grid_size == 128
    (dev,), (host,) = _check(g3, synth, [0.1], [first, second], free=2)
    assert dev.grid_size == host.grid_size == 256


# ---- 8. errors the device finds -------------------------------------------------------------
def test_errors_found_on_the_device_name_the_insertion_and_change_no_grid(g3, synth):
    from cartographer_amd import _lib
    rng = np.random.default_rng(23)
    grids = [g3.HybridGridOnDevice(r) for r in (0.1, 0.45, 0.1, 0.45)]
    origin = np.zeros(3, np.float32)
    clouds = [rng.uniform(-2.0, 2.0, (40, 3)).astype(np.float32) for _ in grids]
    g3.insert_batch([(g, origin, c) for g, c in zip(grids, clouds)], num_free_space_voxels=2)
    before = [(g.grid_size, g.voxels()) for g in grids]

    def unchanged():
        for grid, (size, voxels) in zip(grids, before):
            assert grid.grid_size == size
            np.testing.assert_array_equal(grid.voxels(), voxels)

    # a ray of 40 000 voxels in insertion 2 of 4; the others would grow their bricks
    wide = [(c * 4).astype(np.float32) for c in clouds]
    long_ray = wide[2].copy()
    long_ray[17] = (4000.0, 0.0, 0.0)
    with pytest.raises(_lib.CmxError) as e:
        g3.insert_batch([(grids[0], origin, wide[0]), (grids[1], origin, wide[1]),
                         (grids[2], origin, long_ray), (grids[3], origin, wide[3])],
                        num_free_space_voxels=2)
    assert e.value.status == _lib.INVALID_ARGUMENT
    assert "insertion 2" in str(e.value) and "2^15" in str(e.value)
    unchanged()
    # a voxel index of 1.1e6 (beyond 2^20) at the end of a short ray, in insertion 1
    far_origin = np.array([110000.0, 0.0, 0.0], np.float32)
    far = np.array([[110001.0, 0.0, 0.0]], np.float32)
    with pytest.raises(_lib.CmxError) as e:
        g3.insert_batch([(grids[1], origin, wide[1]), (grids[0], far_origin, far),
                         (grids[2], origin, wide[2]), (grids[3], origin, wide[3])],
                        num_free_space_voxels=2)
    assert e.value.status == _lib.INVALID_ARGUMENT
    assert "insertion 1" in str(e.value) and "out of range" in str(e.value)
    unchanged()
    # the list without the bad return goes through, and equals the single calls
    g3.insert_batch([(g, origin, w) for g, w in zip(grids, wide)], num_free_space_voxels=2)
    for grid, res, cloud, w in zip(grids, (0.1, 0.45, 0.1, 0.45), clouds, wide):
        host = synth.HybridGrid(res)
        host.insert(origin, cloud, 0.7, 0.4, 2)
        host.insert(origin, w, 0.7, 0.4, 2)
        assert grid.grid_size == host.grid_size
        np.testing.assert_array_equal(grid.voxels(), host.voxels())


# ---- 9. two devices -------------------------------------------------------------------------
def test_grids_on_two_devices_in_one_call_are_invalid(g3):
    from cartographer_amd import _lib
    if _lib.lib().cmx_device_count() < 2:
        pytest.skip("needs two HIP devices: a grid each")
    grids = [g3.HybridGridOnDevice(0.1, device=0), g3.HybridGridOnDevice(0.1, device=1)]
    origin = np.zeros(3, np.float32)
    cloud = np.ones((5, 3), np.float32)
    with pytest.raises(_lib.CmxError) as e:
        g3.insert_batch([(g, origin, cloud) for g in grids])
    assert e.value.status == _lib.INVALID_ARGUMENT and "insertion 1" in str(e.value)
    assert all(len(g.voxels()) == 0 for g in grids)
