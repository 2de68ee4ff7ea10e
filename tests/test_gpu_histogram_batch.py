"""cmx_compute_histogram_batch on the device: every job bit for bit the single call
(filters.compute_histogram) on the same array and, wherever the oracle's order is determined,
the oracle -- sizes around every boundary of the one-workgroup kernel (the wavefront, the LDS
carves, the single route), one slice holding a whole cloud, clouds without a surviving point,
exact duplicates, distinct points of equal angle (the stable order), lidar-shaped clouds, a mixed
fleet with shared, empty, large and non-finite clouds, a call cut into sets, and an argument error
in the middle of a list."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = [(1, 120, 1.0), (2, 7, 0.3), (63, 1, 2.0), (64, 120, 0.5), (65, 16, 0.5), (1000, 120, 4.0),
        (2048, 120, 3.0), (2049, 120, 3.0), (4096, 120, 6.0), (4096, 8192, 3.0), (4097, 120, 3.0)]
# the oracle's histogram sums for ROWS
ROW_SUMS = [0.0, 1.2e-7, 2.9, 15.4, 21.1, 31.9, 39.2, 41.0, 53.9, 49.8, 35.8]


def _blob(n, size, spread):
    rng = np.random.default_rng(n + size)
    return (rng.normal(0.0, spread, (n, 3)) * np.array([1.0, 1.0, 0.15])).astype(np.float32)


def _ring(n):
    """A one-slice scan of an 8 m x 6 m room from (0.7, -0.4): n rays at random bearings."""
    rng = np.random.default_rng(5)
    bearing = rng.uniform(-np.pi, np.pi, n)
    c, s = np.cos(bearing), np.sin(bearing)
    ox, oy = 0.7, -0.4
    with np.errstate(divide="ignore"):
        tx = np.where(c > 0, (4.0 - ox) / c, (-4.0 - ox) / c)
        ty = np.where(s > 0, (3.0 - oy) / s, (-3.0 - oy) / s)
    r = np.minimum(tx, ty) + rng.normal(0.0, 0.01, n)
    return np.stack([r * c, r * s, np.full(n, 0.05)], axis=1).astype(np.float32)


def _duplicates(k):
    rng = np.random.default_rng(77 + k)
    cloud = (rng.normal(0.0, 3.0, (2000, 3)) * np.array([1.0, 1.0, 0.15])).astype(np.float32)
    cloud[::7][:k] = cloud[1::7][:k]
    return cloud


def _equal_angles():
    rng = np.random.default_rng(11)
    pts = []
    for i in range(48):
        p = (5.0, rng.integers(-255, 256) / 64.0) if i % 2 == 0 else \
            (rng.integers(-319, 320) / 64.0, 4.0)
        q = (p[0] * 15 / 16, p[1] * 15 / 16)
        for w in ((p, q) if i % 3 else (q, p)):
            pts += [(w[0], w[1], 0.05), (-w[0], -w[1], 0.05)]
    return np.array(pts, np.float32)    # 192 points, x and y exact in f32


def _check(oracle, clouds, sizes, got, with_oracle=True):
    from cartographer_amd import filters
    assert len(got) == len(clouds)
    singles = []
    for k, (cloud, size) in enumerate(zip(clouds, sizes)):
        single = filters.compute_histogram(cloud, size)
        assert got[k].dtype == np.float32 and got[k].shape == (size,)
        np.testing.assert_array_equal(got[k], single, err_msg=f"job {k} against the single call")
        flags = with_oracle if isinstance(with_oracle, (list, tuple)) else [with_oracle] * len(clouds)
        if flags[k]:
            np.testing.assert_array_equal(got[k], oracle.compute_histogram(cloud, size),
                                          err_msg=f"job {k} against the oracle")
        singles.append(single)
    return singles


def test_sizes_around_every_boundary_in_one_call(oracle):
    from cartographer_amd import filters
    clouds = [np.zeros((0, 3), np.float32)] + [_blob(*row) for row in ROWS]
    sizes = [120] + [row[1] for row in ROWS]
    plans, call = filters.histogram_batch_plan(clouds, sizes)
    assert [p["route"] for p in plans] == [0] + [1] * 10 + [2]
    got = filters.compute_histogram_batch(clouds, sizes)
    singles = _check(oracle, clouds, sizes, got)
    assert not got[0].any()
    # the cases are the ones they were chosen to be
    for single, want in zip(singles[1:], ROW_SUMS):
        assert single.sum(dtype=np.float64) == pytest.approx(want, rel=0.05), (single.sum(), want)


@pytest.mark.parametrize("n,total,buckets", [(4096, 2012.5, 48), (1000, 500.6, 51)])
def test_one_slice_with_many_votes_and_long_chains(oracle, n, total, buckets):
    from cartographer_amd import filters
    cloud = _ring(n)
    got = filters.compute_histogram_batch([cloud], 120)
    single, = _check(oracle, [cloud], [120], got)
    # (the oracle's figures for these bearings: one slice, every vote in a few dozen buckets)
    assert single.sum(dtype=np.float64) == pytest.approx(total, abs=0.1)
    assert np.count_nonzero(single) == buckets


def test_one_slice_around_the_line_between_the_two_walks(oracle):
    """A slice of fewer than 256 kept points is walked by one lane, a longer one by a wavefront
    64 points at a time: rings (nothing dropped, one slice) on both sides of the line, and one that
    fills a window exactly."""
    from cartographer_amd import filters
    clouds = [_ring(n) for n in (255, 256, 257, 320)]
    got = filters.compute_histogram_batch(clouds, 120)
    singles = _check(oracle, clouds, [120] * 4, got)
    assert all(s.sum() > 50 for s in singles)


def test_nothing_survives(oracle):
    from cartographer_amd import filters
    rng = np.random.default_rng(3000)
    cloud = (rng.normal(0.0, 0.05, (3000, 3)) * np.array([1.0, 1.0, 0.15])).astype(np.float32)
    got = filters.compute_histogram_batch([cloud], 120)
    _check(oracle, [cloud], [120], got)
    assert not got[0].any()


def test_exact_duplicates(oracle):
    from cartographer_amd import filters
    clouds = [_duplicates(k) for k in (1, 40, 285)]
    got = filters.compute_histogram_batch(clouds, 120)
    singles = _check(oracle, clouds, [120] * 3, got)
    assert all(s.sum() > 0 for s in singles)


def test_equal_angles_of_distinct_points_keep_the_single_calls_order(oracle):
    """Pairs p, 15/16 p have the same atan2f around a centroid of exactly 0: the order inside a
    tie decides 45 buckets.  The oracle's std::sort is unstable and matches neither order; the
    single call's is ascending input index, and so must the batch's be."""
    from cartographer_amd import filters
    cloud = _equal_angles()
    assert cloud.shape == (192, 3)
    single = filters.compute_histogram(cloud, 120)
    assert (oracle.compute_histogram(cloud, 120) != single).any()
    got = filters.compute_histogram_batch([cloud], 120)
    _check(oracle, [cloud], [120], got, with_oracle=False)
    assert single.sum() > 0


def _lidar(synth, seed):
    grid, world = synth.make_submap_3d(20 + seed, 0.1, (8.0, 6.0, 3.0), 4, 10, 64)
    pos = world.free_position(seed, 0.5)
    return world.scan(pos, 0.2 * seed, 11, 360, seed=seed)


def test_lidar_shaped_clouds(oracle, synth):
    from cartographer_amd import filters
    clouds = [_lidar(synth, seed) for seed in (0, 1, 2)]
    assert all(len(c) == 3960 for c in clouds)
    plans, call = filters.histogram_batch_plan(clouds, 120)
    assert [p["route"] for p in plans] == [1, 1, 1]
    got = filters.compute_histogram_batch(clouds, 120)
    singles = _check(oracle, clouds, [120] * 3, got)
    assert all(s.sum() > 0 for s in singles)


def _fleet(synth):
    """16 jobs in shuffled order: (cloud, size, compared with the oracle); and the cloud that two
    of them share."""
    shared = _blob(1000, 120, 4.0)
    poisoned = _blob(300, 120, 2.0)
    poisoned[17, 2] = np.nan
    jobs = [(_blob(*row), row[1], True) for row in ROWS[:9]]
    jobs += [(shared, 120, True), (shared, 7, True),
             (np.zeros((0, 3), np.float32), 33, True),
             (_blob(5000, 120, 4.0), 120, True),
             (poisoned, 120, False),
             (_ring(1000), 120, True), (_lidar(synth, 1), 120, True)]
    assert len(jobs) == 16
    order = np.random.default_rng(16).permutation(16)
    return [jobs[i] for i in order], shared


def test_a_mixed_fleet_in_one_call(oracle, synth):
    from cartographer_amd import filters
    jobs, shared = _fleet(synth)
    clouds, sizes, flags = [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs]
    plans, call = filters.histogram_batch_plan(clouds, sizes)
    assert sorted(p["route"] for p in plans) == [0] + [1] * 13 + [2] * 2
    slots = [p["cloud_slot"] for p, c in zip(plans, clouds) if c is shared]
    assert len(slots) == 2 and slots[0] == slots[1]
    assert len({p["cloud_slot"] for p in plans}) == 15      # 14 distinct clouds and the empty one's -1
    got = filters.compute_histogram_batch(clouds, sizes)
    _check(oracle, clouds, sizes, got, with_oracle=flags)


def test_a_call_in_several_sets_returns_the_same(oracle, synth, debug):
    from cartographer_amd import filters
    jobs, shared = _fleet(synth)
    clouds, sizes = [j[0] for j in jobs], [j[1] for j in jobs]
    whole = filters.compute_histogram_batch(clouds, sizes)
    debug(histogram_batch_set_kb=64)
    plans, call = filters.histogram_batch_plan(clouds, sizes)
    assert call["num_sets"] >= 2
    parts = filters.compute_histogram_batch(clouds, sizes)
    for k, (a, b) in enumerate(zip(whole, parts)):
        np.testing.assert_array_equal(a, b, err_msg=f"job {k}")
    _check(oracle, clouds, sizes, parts, with_oracle=False)


def test_an_argument_error_in_the_middle_leaves_every_output_untouched():
    from cartographer_amd import _lib
    clouds = [_blob(100 + k, 120, 2.0) for k in range(5)]
    outputs = [np.full(120, -7.0, np.float32) for _ in range(5)]
    items = (_lib.HistogramJob * 5)()
    for k in range(5):
        items[k].point_cloud_xyz, items[k].num_points = clouds[k].ctypes.data, len(clouds[k])
        items[k].histogram_size, items[k].histogram = 120, outputs[k].ctypes.data
    items[2].histogram_size = 8193
    assert _lib.lib().cmx_compute_histogram_batch(items, 5, 0) == _lib.INVALID_ARGUMENT
    assert "job 2" in _lib.lib().cmx_last_error().decode()
    assert all((out == -7.0).all() for out in outputs)
    items[2].histogram_size = 120
    assert _lib.lib().cmx_compute_histogram_batch(items, 5, 0) == _lib.OK
    assert all((out != -7.0).all() for out in outputs)
