"""What the probability-grid insertion kernels do on their own, compared bit for bit.

1. The ray mask.  ForEachRayPixel (csrc/ray_mask_2d.h) is a closed form per pixel column over the
   64 lanes of a wavefront, not the reference's incremental RayToPixelMask.  The integer rays of
   tests/ray_mask_cases.py -- every exact-corner ray of a sweep, rays of 64 / 65 / 128 / 129
   columns, single-column rays of more than 64 rows, lattice slopes -- reach GridMissKernel and
   BatchMissKernel as exact float32 points through `insert` and `insert_batch`, one ray per
   insertion, each in a tile of its own: the non-zero cells of a tile are the ray's mask, and every
   one of them holds the miss table's value for an unknown cell, so it was written once.
2. The odds table the kernels apply (OddsTable in csrc/grid_2d.hip, also behind the batch call):
   a grid created with the cells 0 .. 32767 in order, every cell hit (or crossed by a ray) once,
   equals synth.odds_table entry by entry, the clamped ends included; and eighty applications of
   one ray hold the clamp.
3. cmx_grid2d_create accepts the cells it should (the refusal of marked cells is in test_abi.py).

The host side of every comparison is synth.ProbabilityGrid / synth.cells_on_ray / synth.odds_table,
which tests/test_ray_mask_cases.py, tests/test_reference_ref.py and tests/test_reference_ref_grid.py
pin to the reference.

The limit of this.  The four TSDF owner and apply kernels inline the same header, but take their
ray ends from float geometry computed on the host (the ray is lengthened by the truncation
distance along its direction), which cannot be made exact except along the axes: no integer ray
can be aimed at them through the public calls.  Their side stays pinned by the TSDF goldens
(tests/test_gpu_tsdf.py, tests/test_gpu_tsdf2d_insert_batch.py).
"""
import numpy as np
import pytest

import ray_mask_cases as rc

pytestmark = pytest.mark.gpu

HIT, MISS = 0.7, 0.4
EMPTY = np.zeros((0, 3), np.float32)
BATCH_GRIDS = {"sweep": 64, "structured": 6}     # 36 and 42 rounds in one call
SINGLE_GRIDS = {"sweep": 1, "structured": 4}


@pytest.fixture(scope="module")
def g2():
    from cartographer_amd import _lib, grid_2d
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return grid_2d


def _limits(nx, ny):
    return dict(resolution=rc.RESOLUTION, max_x=rc.MAX_XY, max_y=rc.MAX_XY, num_x_cells=nx,
                num_y_cells=ny)


def _device_grid(g2, nx, ny, cells=None):
    return g2.ProbabilityGridOnDevice(rc.RESOLUTION, (rc.MAX_XY, rc.MAX_XY), nx, ny, cells=cells)


def _host_grid(synth, nx, ny):
    return synth.ProbabilityGrid(rc.RESOLUTION, (rc.MAX_XY, rc.MAX_XY), nx, ny)


# ---- 1. the ray mask ----------------------------------------------------------------------------
class _Expected:
    """A layout of one family of rays with what the host makes of it; computed once per layout,
    read only afterwards."""

    def __init__(self, synth, family, grids):
        rays = rc.sweep_cases() if family == "sweep" else rc.structured_cases()
        self.layout = rc.pack(rays, grids)
        placed = self.layout.placed
        self.origins = rc.points_of([p.begin for p in placed])[:, :2].copy()
        self.ends = rc.points_of([p.end for p in placed])
        self.masks = [np.zeros((ny, nx), bool) for nx, ny in self.layout.sizes]
        hosts = [_host_grid(synth, nx, ny) for nx, ny in self.layout.sizes]
        for k, p in enumerate(placed):
            hosts[p.grid].insert(self.origins[k], EMPTY, self.ends[k:k + 1], HIT, MISS, True)
            on_ray = synth.cells_on_ray(p.begin, p.end, rc.SCALE)
            w, h = p.ray.tile                       # the mask stays inside the ray's own tile
            assert (on_ray[:, 0] > p.x).all() and (on_ray[:, 0] < p.x + w - 1).all(), p.ray.name
            assert (on_ray[:, 1] > p.y).all() and (on_ray[:, 1] < p.y + h - 1).all(), p.ray.name
            self.masks[p.grid][on_ray[:, 1], on_ray[:, 0]] = True
        self.host_limits = [h.limits for h in hosts]
        self.host_cells = [h.cells for h in hosts]
        for cells, mask in zip(self.host_cells, self.masks):
            cells.setflags(write=False)
            mask.setflags(write=False)
        self.miss_value = int(synth.odds_table(MISS)[0]) - 32768
        assert 0 < self.miss_value < 32768


_expected_cache = {}


def _expected(synth, family, grids):
    key = (family, grids)
    if key not in _expected_cache:
        _expected_cache[key] = _Expected(synth, family, grids)
    return _expected_cache[key]


def _check_masks(want, devices):
    layout = want.layout
    cells = [d.cells for d in devices]
    for g, d in enumerate(devices):
        assert d.limits == want.host_limits[g] == _limits(*layout.sizes[g]), g
        assert not (cells[g] & 0x8000).any(), "grid %d keeps update markers at (y, x) %s" % (
            g, np.argwhere(cells[g] & 0x8000)[:5].tolist())
    for p in layout.placed:                              # tile by tile: the failing ray is named
        w, h = p.ray.tile
        window = (slice(p.y, p.y + h), slice(p.x, p.x + w))
        got, mask = cells[p.grid][window] != 0, want.masks[p.grid][window]
        if not np.array_equal(got, mask):
            here = np.array([p.x, p.y])
            raise AssertionError(
                "ray %s %s -> %s (grid %d, tile at pixel %d, %d): pixels (x, y) missing %s, "
                "not of the ray %s" % (p.ray.name, p.ray.begin, p.ray.end, p.grid, p.x, p.y,
                                       (np.argwhere(mask & ~got)[:, ::-1] - here).tolist(),
                                       (np.argwhere(got & ~mask)[:, ::-1] - here).tolist()))
    for g in range(len(devices)):
        # nothing outside the tiles' masks, every cell written once, and all of it the host's grid
        np.testing.assert_array_equal(cells[g] != 0, want.masks[g], err_msg="grid %d" % g)
        wrong = np.argwhere((cells[g] != 0) & (cells[g] != want.miss_value))
        assert wrong.size == 0, "grid %d: cells (y, x) %s hold %s, not %d" % (
            g, wrong[:5].tolist(), [int(cells[g][tuple(c)]) for c in wrong[:5]], want.miss_value)
        np.testing.assert_array_equal(cells[g], want.host_cells[g], err_msg="grid %d" % g)


@pytest.mark.parametrize("family", ["sweep", "structured"])
def test_ray_mask_single_call(g2, synth, family):
    """One cmx_grid2d_insert per ray (GridMissKernel): 2266 sweep rays tiled into one grid, the
    structured rays into four."""
    want = _expected(synth, family, SINGLE_GRIDS[family])
    devices = [_device_grid(g2, nx, ny) for nx, ny in want.layout.sizes]
    for k, p in enumerate(want.layout.placed):
        devices[p.grid].insert(want.origins[k], EMPTY, want.ends[k:k + 1], HIT, MISS, True)
    _check_masks(want, devices)


@pytest.mark.parametrize("chain", [0, 5])
@pytest.mark.parametrize("family", ["sweep", "structured"])
def test_ray_mask_batch_call(g2, synth, debug, family, chain):
    """The same rays through one cmx_grid2d_insert_batch (BatchMissKernel), dealt over several
    grids so that the call has tens of rounds; chain = 5 cuts every round into sets of launches of
    at most five insertions.  No cell may keep bit 15: the only check that the box
    BatchFinishKernel sweeps contains everything a ray marks."""
    if chain:
        debug(grid2d_insert_chain=chain)
    want = _expected(synth, family, BATCH_GRIDS[family])
    devices = [_device_grid(g2, nx, ny) for nx, ny in want.layout.sizes]
    ends = [want.ends[k:k + 1] for k in range(len(want.layout.placed))]
    g2.insert_batch([(devices[p.grid], want.origins[k], None, ends[k])
                     for k, p in enumerate(want.layout.placed)], HIT, MISS, True)
    _check_masks(want, devices)


# ---- 2. every cell value ------------------------------------------------------------------------
NX, NY = 256, 128                                  # 32768 cells: every value once
HITS = (0.55, 0.7, 0.9, 0.999)
MISSES = (0.49, 0.4, 0.1, 0.001)


def _centres(cells_xy):
    return rc.points_of(np.asarray(cells_xy, np.int64) * rc.SCALE + rc.SCALE // 2)


def _host_from_cells(synth, oracle, cells):
    """synth.ProbabilityGrid holding `cells`: SetProbability(1 - cost of the value) on the unknown
    grid gives every value back (the identity tests/test_device_formulas.py pins); checked."""
    ny, nx = cells.shape
    host = _host_grid(synth, nx, ny)
    value_to_cost = oracle.value_tables()[1]
    for iy, ix in np.argwhere(cells != 0):
        host.set_probability(int(ix), int(iy), float(np.float32(1) - value_to_cost[cells[iy, ix]]))
    np.testing.assert_array_equal(host.cells, cells)
    return host


@pytest.fixture(scope="module")
def all_values():
    cells = np.arange(NX * NY, dtype=np.uint16).reshape(NY, NX)
    assert cells.max() == 32767
    cells.setflags(write=False)
    return cells


@pytest.fixture(scope="module")
def every_cell_once():
    """(returns at every cell centre; origin in the middle and a miss in every border cell)."""
    xs, ys = np.meshgrid(np.arange(NX), np.arange(NY))
    every = _centres(np.stack([xs.ravel(), ys.ravel()], 1))
    border = [(x, y) for x in range(NX) for y in (0, NY - 1)]
    border += [(x, y) for y in range(1, NY - 1) for x in (0, NX - 1)]
    assert len(set(border)) == len(border) == 2 * NX + 2 * NY - 4
    return every, _centres([(NX // 2, NY // 2)])[0, :2].copy(), _centres(border)


def _insert(g2, how, grid, origin, returns, misses, hit, miss, free):
    if how == "batch":
        g2.insert_batch([(grid, origin, returns, misses)], hit, miss, free)
    else:
        grid.insert(origin, EMPTY if returns is None else returns, misses, hit, miss, free)


@pytest.mark.parametrize("how", ["single", "batch"])
@pytest.mark.parametrize("probability", HITS)
def test_hit_table_on_every_cell_value(g2, synth, oracle, all_values, every_cell_once, how,
                                       probability):
    """One return at every cell centre, no free space, one insertion: cell v becomes
    odds_table(p)[v] without the marker, v = 0 (unknown) and the clamped top included."""
    every, origin, _ = every_cell_once
    dev = _device_grid(g2, NX, NY, all_values)
    host = _host_from_cells(synth, oracle, all_values)
    _insert(g2, how, dev, origin, every, None, probability, MISS, False)
    host.insert(origin, every, None, probability, MISS, False)
    got = dev.cells
    table = synth.odds_table(probability)
    assert (table >= 32768).all()
    np.testing.assert_array_equal(got, (table[all_values] - 32768).astype(np.uint16))
    assert dev.limits == host.limits == _limits(NX, NY)
    np.testing.assert_array_equal(got, host.cells)


@pytest.mark.parametrize("how", ["single", "batch"])
@pytest.mark.parametrize("probability", MISSES)
def test_miss_table_on_every_cell_value(g2, synth, oracle, all_values, every_cell_once, how,
                                        probability):
    """Misses only, from the middle to every border cell: the rays cross every cell of the grid
    (on the host restatement: the same insertion into unknown cells leaves none unknown), each is
    updated once, so cell v becomes odds_table(p)[v] without the marker."""
    _, origin, border = every_cell_once
    covered = _host_grid(synth, NX, NY)
    covered.insert(origin, EMPTY, border, HIT, probability, True)
    assert (covered.cells != 0).all(), "the rays leave cells untouched"
    dev = _device_grid(g2, NX, NY, all_values)
    host = _host_from_cells(synth, oracle, all_values)
    _insert(g2, how, dev, origin, None, border, HIT, probability, True)
    host.insert(origin, EMPTY, border, HIT, probability, True)
    got = dev.cells
    table = synth.odds_table(probability)
    np.testing.assert_array_equal(got, (table[all_values] - 32768).astype(np.uint16))
    assert dev.limits == host.limits == _limits(NX, NY)
    np.testing.assert_array_equal(got, host.cells)


@pytest.mark.parametrize("how", ["single", "batch"])
def test_eighty_misses_along_one_row_reach_the_clamp_and_hold_it(g2, synth, oracle, how):
    """One ray along the middle row of a 70 x 3 grid whose cells span the value range, applied
    eighty times: compared with the host after every tenth application (through the batch call:
    ten insertions of one grid, ten rounds, per call).  Every cell of the ray ends at the largest
    correspondence cost, 32767, and stays there."""
    nx, ny = 70, 3
    start = np.zeros((ny, nx), np.uint16)
    start[1] = np.linspace(0, 32767, nx).astype(np.uint16)
    start[1, 1], start[1, 2] = 1, 32767                 # both ends of the range on the ray
    dev = _device_grid(g2, nx, ny, start)
    host = _host_from_cells(synth, oracle, start)
    origin, end = _centres([(1, 1)])[0, :2].copy(), _centres([(nx - 2, 1)])
    on_ray = np.zeros((ny, nx), bool)
    on_ray[1, 1:nx - 1] = True
    held = None
    for tenth in range(8):
        if how == "batch":
            g2.insert_batch([(dev, origin, None, end)] * 10, HIT, MISS, True)
        for _ in range(10):
            host.insert(origin, EMPTY, end, HIT, MISS, True)
            if how == "single":
                dev.insert(origin, EMPTY, end, HIT, MISS, True)
        got = dev.cells
        np.testing.assert_array_equal(got, host.cells, err_msg="after %d" % (10 * tenth + 10))
        np.testing.assert_array_equal(got[~on_ray], start[~on_ray])
        if (got[on_ray] == 32767).all():
            held = held or 10 * tenth + 10
    assert held is not None and held <= 40, held        # reached with half the applications to go
    assert (dev.cells[on_ray] == 32767).all()


# ---- 3. the cells cmx_grid2d_create takes -------------------------------------------------------
def test_cells_below_the_marker_are_accepted_and_marked_ones_refused(g2):
    from cartographer_amd import _lib
    cells = (np.arange(16 * 12, dtype=np.uint16) * 171 % 32768).reshape(12, 16)
    cells[0, 0], cells[11, 15] = 0, 32767
    dev = g2.ProbabilityGridOnDevice(0.05, (1.0, 1.0), 16, 12, cells=cells)
    np.testing.assert_array_equal(dev.cells, cells)
    marked = cells.copy()
    marked[7, 3] |= 0x8000
    with pytest.raises(_lib.CmxError) as e:
        g2.ProbabilityGridOnDevice(0.05, (1.0, 1.0), 16, 12, cells=marked)
    assert e.value.status == _lib.INVALID_ARGUMENT and "(x 3, y 7)" in str(e.value)
