"""cmx_grid2d_insert_batch on the device: range data into many resident probability grids in one
call must leave every grid -- limits and every cell -- exactly as the same insertions made one by
one leave it.  Every comparison is made twice: against synth.ProbabilityGrid (the host restatement
of the reference's inserter that tests/test_reference_ref_grid.py pins to the reference) and
against a second set of device grids filled by single cmx_grid2d_insert calls.  No downloaded cell
may keep the update marker (bit 15)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g2():
    from cartographer_amd import _lib, grid_2d
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return grid_2d


def _spec(resolution, max_x, max_y, nx, ny):
    return dict(resolution=resolution, max_x=max_x, max_y=max_y, num_x_cells=nx, num_y_cells=ny)


def _make(kind, spec):
    return kind(spec["resolution"], (spec["max_x"], spec["max_y"]), spec["num_x_cells"],
                spec["num_y_cells"])


def _check(g2, synth, specs, insertions, hit=0.7, miss=0.4, free=True, calls=None):
    """`insertions` = (grid index, origin, returns, misses or None).  One batch call (or one per
    slice of `calls`) into one set of device grids, single calls into a second set and into host
    grids; returns the batch grids."""
    batch = [_make(g2.ProbabilityGridOnDevice, s) for s in specs]
    single = [_make(g2.ProbabilityGridOnDevice, s) for s in specs]
    host = [_make(synth.ProbabilityGrid, s) for s in specs]
    for part in calls or [slice(None)]:
        g2.insert_batch([(batch[g], o, r, m) for g, o, r, m in insertions[part]], hit, miss, free)
    for g, origin, returns, misses in insertions:
        empty = np.zeros((0, 3), np.float32)
        single[g].insert(origin, empty if returns is None else returns, misses, hit, miss, free)
        host[g].insert(origin, empty if returns is None else returns, misses, hit, miss, free)
    for k, (b, s, h) in enumerate(zip(batch, single, host)):
        assert b.limits == h.limits, k
        assert s.limits == h.limits, k
        cells = b.cells
        assert not (cells & 0x8000).any(), k
        np.testing.assert_array_equal(cells, h.cells, err_msg=f"grid {k} against the host")
        np.testing.assert_array_equal(cells, s.cells, err_msg=f"grid {k} against single calls")
    return batch


def _points(rng, n, reach):
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, :2] = rng.uniform(-reach, reach, (n, 2))
    return xyz


# ---- the reference's own fixture ----------------------------------------------------------------
class _View:
    """Gives the reference-test checker of test_oracle_reference_pins the surface it reads."""

    def __init__(self, dev, oracle):
        self._dev = dev
        self._v2c = oracle.value_tables()[1]        # kValueToCorrespondenceCost

    limits = property(lambda self: self._dev.limits)
    cells = property(lambda self: self._dev.cells)

    def get_probability(self, ix, iy):              # probability_grid.cc:78-83
        return float(np.float32(1) - self._v2c[self._dev.cells[iy, ix]])


def test_reference_fixture_through_a_batch_of_one_and_three_rounds_on_one_grid(g2, synth, oracle):
    """RangeDataInserterTest2D.InsertPointCloud (mapping/2d/range_data_inserter_2d_test.cc:65-105)
    through a batch of one; then three more insertions of the fixture in ONE call: three rounds on
    one grid."""
    from test_oracle_reference_pins import (INSERTER_2D_ORIGIN, INSERTER_2D_RETURNS,
                                            check_inserter_2d_fixture)
    spec = [_spec(1.0, 1.0, 5.0, 5, 5)]
    one = [(0, INSERTER_2D_ORIGIN, INSERTER_2D_RETURNS, None)]
    (dev,) = _check(g2, synth, spec, one)
    check_inserter_2d_fixture(_View(dev, oracle))
    _check(g2, synth, spec, one * 4, calls=[slice(0, 1), slice(1, 4)])


# ---- one scan into two grids ----------------------------------------------------------------
@pytest.fixture(scope="module")
def scan_in_map(synth):
    """257 rays of a simulated room in the map frame, and where they were taken from."""
    _, _, world = synth.make_submap(7, 200, 200, 0.05, 12, 500, 30.0, 0.01)
    at = world.free_pose(20, 0.5)
    pts = world.scan(at, 257, 30.0, 0.01, 3).astype(np.float64)
    assert pts.shape[0] == 257
    c, s = np.cos(at[2]), np.sin(at[2])
    in_map = np.zeros((257, 3), np.float32)
    in_map[:, 0] = at[0] + c * pts[:, 0] - s * pts[:, 1]
    in_map[:, 1] = at[1] + s * pts[:, 0] + c * pts[:, 1]
    return at, in_map


def test_one_scan_into_two_grids_by_the_same_pointers(g2, synth, scan_in_map):
    """The ActiveSubmaps2D case: the same array object twice (one pointer, one upload) into a
    16 x 16 grid that must grow and a 100 x 100 grid that must not."""
    at, in_map = scan_in_map
    specs = [_spec(0.05, at[0] + 0.4, at[1] + 0.4, 16, 16),
             _spec(0.2, at[0] + 10.0, at[1] + 10.0, 100, 100)]
    batch = _check(g2, synth, specs, [(0, at[:2], in_map, None), (1, at[:2], in_map, None)])
    assert batch[0].limits["num_x_cells"] > 16
    assert batch[1].limits == specs[1]


# ---- a mixed list ---------------------------------------------------------------------------
MIXED_SPECS = [_spec(0.05, 2.5, 2.5, 100, 100), _spec(0.1, 3.2, 3.2, 64, 64),
               _spec(1.0, 2.5, 2.5, 5, 5), _spec(0.05, 0.4, 0.4, 16, 16),
               _spec(0.1, 2.0, 1.5, 30, 40)]
MIXED_REACH = [3.0, 3.0, 2.0, 1.5, 2.5]
# (grid, returns, misses): five grids with 4, 3, 2, 1 and 2 insertions, interleaved.  Round 0 is
# the insertions 0, 1, 2, 4, 5: one point next to 257 -- the smallest shape at which a wrong block
# table crosses insertions.  Insertion 5 has misses only, insertion 6 neither returns nor misses.
MIXED_LIST = [(0, 1, 0), (1, 257, 0), (2, 4, 0), (0, 255, 5), (3, 256, 0), (4, 0, 5), (1, 0, 0),
              (0, 257, 0), (2, 1, 0), (1, 5, 4), (4, 256, 0), (0, 4, 1)]


def _mixed():
    rng = np.random.default_rng(11)
    out = []
    for grid, returns, misses in MIXED_LIST:
        reach = MIXED_REACH[grid]
        out.append((grid, rng.uniform(-0.3, 0.3, 2).astype(np.float32),
                    _points(rng, returns, reach) if returns else None,
                    _points(rng, misses, reach) if misses else None))
    return out


@pytest.mark.parametrize("free", [0, 1])
@pytest.mark.parametrize("hit,miss", [(0.55, 0.49), (0.7, 0.4)])
def test_mixed_list_equals_the_single_calls(g2, synth, hit, miss, free):
    from cartographer_amd import grid_2d
    insertions = _mixed()
    rounds, final = grid_2d.insert_batch_plan(MIXED_SPECS, insertions)
    assert rounds == [0, 0, 0, 1, 0, 0, 1, 2, 1, 2, 1, 3]
    batch = _check(g2, synth, MIXED_SPECS, insertions, hit, miss, bool(free))
    assert [b.limits for b in batch] == final                 # the launch path asked the same plan
    assert batch[0].limits["num_x_cells"] > 100 and batch[3].limits["num_x_cells"] > 16


@pytest.mark.parametrize("chain", [1, 2])
def test_rounds_cut_into_sets_of_launches_give_the_same_cells(g2, synth, debug, chain):
    """grid2d_insert_chain: a round of five insertions goes out as five (three) sets of launches."""
    debug(grid2d_insert_chain=chain)
    _check(g2, synth, MIXED_SPECS, _mixed())


# ---- growth in the middle of a call ---------------------------------------------------------
def test_a_grid_that_first_grows_at_its_third_insertion_of_the_call(g2, synth):
    """The first two insertions are made with the 16 x 16 limits into storage that already has the
    final 64 x 64 cells; the third reaches x = 10 m, two doublings away."""
    rng = np.random.default_rng(3)
    far = _points(rng, 6, 3.0)
    far[4, 0] = 10.0
    insertions = [(0, (0.3, -0.2), _points(rng, 9, 3.0), None),
                  (0, (-1.0, 1.0), _points(rng, 7, 3.5), _points(rng, 3, 3.0)),
                  (0, (0.5, 0.5), far, None),
                  (0, (2.0, 2.0), _points(rng, 8, 6.0), None)]
    (grid,) = _check(g2, synth, [_spec(0.5, 4.0, 4.0, 16, 16)], insertions)
    assert grid.limits["num_x_cells"] == 64
    # and with cells from before the call
    before = [(0, (0.0, 0.0), _points(rng, 20, 3.0), None)]
    _check(g2, synth, [_spec(0.5, 4.0, 4.0, 16, 16)], before + insertions,
           calls=[slice(0, 1), slice(1, 5)])


# ---- the real-time matcher's cached image ---------------------------------------------------
def test_a_match_after_a_batch_insertion_sees_the_new_cells(g2, scan_in_map):
    """cmx_rt2d_match_grid keeps a staged image of the grid by its version: after a batch
    insertion the match must equal the match on a fresh device grid made of the downloaded
    cells."""
    from cartographer_amd import scan_matching as sm
    at, in_map = scan_in_map
    c, s = np.cos(at[2]), np.sin(at[2])
    local = np.zeros_like(in_map)                                 # the scan in its own frame
    dx, dy = in_map[:, 0] - at[0], in_map[:, 1] - at[1]
    local[:, 0], local[:, 1] = c * dx + s * dy, -s * dx + c * dy
    grid = g2.ProbabilityGridOnDevice(0.05, (at[0] + 10.0, at[1] + 10.0), 400, 400)
    grid.insert(at[:2], in_map[::4].copy())
    rt = sm.RealTimeCorrelativeScanMatcher2D(0.2, np.deg2rad(3.0), 0.1, 0.1)
    initial = sm.Rigid2d(at[0] + 0.05, at[1] - 0.05, at[2] + 0.01)
    first = rt.match(initial, local, grid)
    other = g2.ProbabilityGridOnDevice(0.05, (at[0] + 10.0, at[1] + 10.0), 400, 400)
    g2.insert_batch([(grid, at[:2], in_map, None), (other, at[:2], in_map, None),
                     (grid, at[:2] + np.float32(0.1), in_map, None)])
    second = rt.match(initial, local, grid)
    lim = grid.limits
    fresh = g2.ProbabilityGridOnDevice(lim["resolution"], (lim["max_x"], lim["max_y"]),
                                       lim["num_x_cells"], lim["num_y_cells"], grid.cells)
    want = rt.match(initial, local, fresh)
    assert second[0] == want[0]
    assert (second[1].x, second[1].y, second[1].theta) == (want[1].x, want[1].y, want[1].theta)
    assert second[0] != first[0]                                  # the cells did change


# ---- an error in the middle of a list -------------------------------------------------------
def test_an_error_in_the_middle_of_a_list_changes_no_grid(g2, scan_in_map):
    """Insertion 1 passes the pointer of insertion 0's returns with another count:
    CMX_INVALID_ARGUMENT naming it, and no grid -- not even the first, which would have grown --
    has other cells or limits than before."""
    from cartographer_amd import _lib
    at, in_map = scan_in_map
    grids = [g2.ProbabilityGridOnDevice(0.05, (at[0] + 0.4, at[1] + 0.4), 16, 16),
             g2.ProbabilityGridOnDevice(0.2, (at[0] + 10.0, at[1] + 10.0), 100, 100)]
    grids[1].insert(at[:2], in_map[::8].copy())
    before = [(g.limits, g.cells) for g in grids]
    origin = np.ascontiguousarray(at[:2], np.float32)
    items = (_lib.Grid2DInsertion * 3)()
    for item, grid, count in zip(items, (grids[0], grids[1], grids[1]), (257, 100, 257)):
        item.grid, item.origin_xy = grid._h, origin.ctypes.data
        item.returns_xyz, item.num_returns = in_map.ctypes.data, count
        item.misses_xyz, item.num_misses = None, 0
    L = _lib.lib()
    assert L.cmx_grid2d_insert_batch(items, 3, 0.7, 0.4, 1) == _lib.INVALID_ARGUMENT
    assert "insertion 1" in L.cmx_last_error().decode()
    for grid, (limits, cells) in zip(grids, before):
        assert grid.limits == limits
        np.testing.assert_array_equal(grid.cells, cells)
    # the same list with the counts put right goes through
    items[1].num_returns = 257
    assert L.cmx_grid2d_insert_batch(items, 3, 0.7, 0.4, 1) == _lib.OK, L.cmx_last_error()
    assert grids[0].limits["num_x_cells"] > 16
