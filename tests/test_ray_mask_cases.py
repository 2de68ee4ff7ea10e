"""The integer rays of tests/ray_mask_cases.py on the CPU: the list is what it claims to be (exact
corners in every class of ray, every structured family, tiles that keep the rays apart), its rays
reach the kernels as the integers they are, and on every one of them the host restatement
(synth.cells_on_ray, what tests/test_gpu_grid_exact.py compares the device with) equals the
reference's own RayToPixelMask.  The conditions below are conditions on the list, not
measurements: a list that misses one is to be mended, not the condition.

The comparison with the reference is skipped where neither the reference tree nor a prebuilt
oracle/_ref/libref.so exists, as in tests/test_reference_ref.py.
"""
import collections

import numpy as np
import pytest

import ray_mask_cases as rc


@pytest.fixture(scope="module")
def ref(oracle):
    lib = oracle.ref_lib()
    if lib is None:
        pytest.skip("reference tree not available and oracle/_ref not prebuilt")
    return lib


def _all_cases():
    return rc.sweep_cases() + rc.structured_cases()


# ---- the list -----------------------------------------------------------------------------------
def test_corner_crossings_on_rays_worked_out_by_hand():
    # the main diagonal from the middle sub-pixel: a corner at each of the three borders
    assert rc.corner_crossings((500, 500), (3500, 3500)) == 3
    assert rc.corner_crossings((3500, 3500), (500, 500)) == 3
    # one sub-pixel off the diagonal: none
    assert rc.corner_crossings((500, 501), (3500, 3501)) == 0
    # the anti-diagonal needs sub-pixels (s, 999 - s)
    assert rc.corner_crossings((499, 3500), (3499, 500)) == 3
    assert rc.corner_crossings((500, 3500), (3500, 500)) == 0
    # axis-aligned rays and rays inside one column cross no corner
    assert rc.corner_crossings((500, 500), (9500, 500)) == 0
    assert rc.corner_crossings((100, 500), (900, 9500)) == 0
    # dy / dx = 2 never does (odd + 2 * odd is odd); 3 from next to a corner does, every column
    assert rc.corner_crossings((500, 500), (4500, 8500)) == 0
    assert rc.corner_crossings((999, 998), (3999, 9998)) == 3
    # one sub-pixel of dx: the border is half way, at 1 + 999 half sub-pixels (the middle of the
    # pixel) for the first ray and at 1999 + 1 (a corner) for the second
    assert rc.corner_crossings((999, 0), (1000, 999)) == 0
    assert rc.corner_crossings((999, 999), (1000, 1000)) == 1


def test_sweep_is_the_full_product_and_keeps_every_exact_corner_ray():
    rays = rc.sweep_all()
    assert len(rays) == 25 * 49 * 64 == 78400
    assert len(set((b, e) for b, e, _ in rays)) == len(rays)
    corner = {(b, e) for b, e, n in rays if n > 0}
    cases = rc.sweep_cases()
    kept_corner = [r for r in cases if r.family == "sweep_corner"]
    sample = [r for r in cases if r.family == "sweep"]
    assert {(r.begin, r.end) for r in kept_corner} == corner
    assert len(kept_corner) == len(corner) >= 600
    assert len(sample) == rc.SWEEP_SAMPLE
    assert len({(r.begin, r.end) for r in sample}) == rc.SWEEP_SAMPLE
    assert all(rc.corner_crossings(r.begin, r.end) == 0 for r in sample)
    assert rc.sweep_cases() is cases                               # built once, seeded


def test_every_class_of_ray_has_its_exact_corners():
    """(listed in x order or reversed) x (dy > 0, dy < 0 once ordered): ForEachRayPixel swaps the
    ends of the first and takes another branch for the second."""
    classes = collections.Counter(rc.corner_class(r.begin, r.end) for r in rc.sweep_cases()
                                  if r.family == "sweep_corner")
    for order in ("given", "reversed"):
        for rise in ("up", "down"):
            assert classes[(order, rise)] >= 150, (order, rise, classes)
    assert sum(classes.values()) == sum(1 for r in rc.sweep_cases() if r.family == "sweep_corner")


def test_every_structured_family_is_present_with_the_spans_and_orders_it_names():
    cases = rc.structured_cases()
    by_family = collections.defaultdict(list)
    for r in cases:
        by_family[r.family].append(r)
    assert set(by_family) == set(rc.STRUCTURED_FAMILIES)
    pixels = lambda r: (abs(r.end[0] // rc.SCALE - r.begin[0] // rc.SCALE),
                        abs(r.end[1] // rc.SCALE - r.begin[1] // rc.SCALE))
    names = {r.name for r in cases}
    for r in cases:                                                # both orders of begin and end
        if r.family != "point":
            other = r.name[:-len("_reversed")] if r.name.endswith("_reversed") else r.name + "_reversed"
            assert other in names, r.name
    for family, want in (("horizontal", lambda n: (n, 0)), ("vertical", lambda n: (0, n)),
                         ("diagonal", lambda n: (n, n)), ("anti_diagonal", lambda n: (n, n)),
                         ("single_column", lambda n: (0, n))):
        spans = collections.Counter(pixels(r) for r in by_family[family])
        assert set(spans) == {want(n) for n in rc.SPANS}, family
    # the lane stride: rays of 64, 65, 128 and 129 columns, single-column rays of more than 64 rows
    columns = {pixels(r)[0] + 1 for r in by_family["horizontal"] + by_family["diagonal"]}
    assert {2, 64, 65, 66, 128, 129, 130, 201} <= columns
    assert max(pixels(r)[1] for r in by_family["single_column"]) + 1 > 64
    assert all(r.begin[0] != r.end[0] for r in by_family["single_column"])
    assert {np.sign(r.end[1] - r.begin[1]) for r in by_family["single_column"]} == {1, -1}
    # diagonals and anti-diagonals: a corner at every border
    for r in by_family["diagonal"] + by_family["anti_diagonal"]:
        assert rc.corner_crossings(r.begin, r.end) == pixels(r)[0], r.name
    # lattice slopes from a pixel centre over 130 columns, four sign combinations, both orders
    assert len(by_family["lattice_slope"]) == 4 * 4 * 2
    for r in by_family["lattice_slope"]:
        assert pixels(r)[0] + 1 == rc.LATTICE_COLUMNS
        first = r.end if r.name.endswith("_reversed") else r.begin
        assert (first[0] % rc.SCALE, first[1] % rc.SCALE) == (rc.SCALE // 2, rc.SCALE // 2)
        assert rc.corner_crossings(r.begin, r.end) == 0            # an even term: never (docstring)
    signs = {(np.sign(r.end[0] - r.begin[0]), np.sign(r.end[1] - r.begin[1]))
             for r in by_family["lattice_slope"] if not r.name.endswith("_reversed")}
    assert signs == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    slopes = {abs(r.end[1] - r.begin[1]) / abs(r.end[0] - r.begin[0])
              for r in by_family["lattice_slope"]}
    assert slopes == {2.0, 0.5, 1.5, 2.0 / 3.0}
    # odd slopes: through corners again and again, rising and falling
    for r in by_family["odd_slope"]:
        assert pixels(r)[0] + 1 >= rc.LATTICE_COLUMNS - 5
        assert rc.corner_crossings(r.begin, r.end) >= 25, r.name
    assert {rc.corner_class(r.begin, r.end) for r in by_family["odd_slope"]} == {
        ("given", "up"), ("given", "down"), ("reversed", "up"), ("reversed", "down")}
    # one sub-pixel of dx across a border
    for r in by_family["one_subpixel_dx"]:
        assert abs(r.end[0] - r.begin[0]) == 1 and pixels(r)[0] == 1
        assert pixels(r)[1] >= 200
        assert rc.corner_crossings(r.begin, r.end) == (1 if "corner" in r.name else 0)
    assert {np.sign(r.end[1] - r.begin[1]) for r in by_family["one_subpixel_dx"]
            if not r.name.endswith("_reversed")} == {1, -1}
    assert all(r.begin == r.end for r in by_family["point"]) and len(by_family["point"]) == 3
    subs = {(r.begin[0] % rc.SCALE, r.begin[1] % rc.SCALE, r.end[0] % rc.SCALE,
             r.end[1] % rc.SCALE) for r in by_family["pixel_edges"]}
    assert len(subs) == 16 and all(s in (0, rc.SCALE - 1) for quad in subs for s in quad)


def test_layouts_keep_every_ray_in_a_tile_of_its_own_inside_a_grid_that_does_not_grow():
    for rays, grids in ((rc.sweep_cases(), 1), (rc.sweep_cases(), 64), (rc.structured_cases(), 4),
                        (rc.structured_cases(), 6)):
        layout = rc.pack(rays, grids)
        assert len(layout.sizes) == grids and len(layout.placed) == len(rays)
        taken = [np.zeros((ny, nx), np.int32) for nx, ny in layout.sizes]
        for k, p in enumerate(layout.placed):
            assert p.ray is rays[k] and p.grid == k % grids
            w, h = p.ray.tile
            nx, ny = layout.sizes[p.grid]
            assert 0 <= p.x and p.x + w <= nx <= rc.MAX_CELLS
            assert 0 <= p.y and p.y + h <= ny <= rc.MAX_CELLS
            taken[p.grid][p.y:p.y + h, p.x:p.x + w] += 1
            # both ends at least one pixel inside the tile: an empty pixel all around
            for end in (p.begin, p.end):
                assert p.x + 1 <= end[0] // rc.SCALE <= p.x + w - 2
                assert p.y + 1 <= end[1] // rc.SCALE <= p.y + h - 2
                assert 0 <= end[0] < rc.MAX_INDEX and 0 <= end[1] < rc.MAX_INDEX
        assert all(t.max() == 1 for t in taken)                    # no two tiles overlap


# ---- the exact points ---------------------------------------------------------------------------
def test_every_superscaled_index_is_a_float32_point_that_comes_back_as_itself():
    """FineIndex's expression in numpy float64 on the float32 point, for every index below
    MAX_INDEX: exactly the index before the rounding, so no rounding mode can matter."""
    index = np.arange(rc.MAX_INDEX, dtype=np.int64)
    exact = rc.MAX_XY - (index + 0.5) * 2.0 ** -13
    point = exact.astype(np.float32)
    assert (point.astype(np.float64) == exact).all()
    assert np.float32(rc.RESOLUTION) == rc.RESOLUTION and rc.RESOLUTION / rc.SCALE == 2.0 ** -13
    back = (rc.MAX_XY - point.astype(np.float64)) / (rc.RESOLUTION / rc.SCALE) - 0.5
    assert (back == index).all()
    # and points_of swaps the axes: cell x from y, cell y from x
    xyz = rc.points_of([(1500, 2500)])
    assert xyz.dtype == np.float32 and xyz.shape == (1, 3)
    assert (rc.MAX_XY - float(xyz[0, 1])) * 2.0 ** 13 - 0.5 == 1500
    assert (rc.MAX_XY - float(xyz[0, 0])) * 2.0 ** 13 - 0.5 == 2500


def test_the_host_inserter_sees_the_rays_as_the_integers_they_are(synth):
    """One miss from each of a few placed rays into synth.ProbabilityGrid: the cells it changes
    are cells_on_ray of the integer ends, so the float points did carry them."""
    rays = rc.structured_cases()[:40] + rc.sweep_cases()[:40]
    layout = rc.pack(rays, 1)
    nx, ny = layout.sizes[0]
    grid = synth.ProbabilityGrid(rc.RESOLUTION, (rc.MAX_XY, rc.MAX_XY), nx, ny)
    want = np.zeros((ny, nx), bool)
    for p in layout.placed:
        grid.insert(rc.points_of([p.begin])[0, :2], np.zeros((0, 3), np.float32),
                    rc.points_of([p.end]), 0.7, 0.4, True)
        on_ray = synth.cells_on_ray(p.begin, p.end, rc.SCALE)
        want[on_ray[:, 1], on_ray[:, 0]] = True
    assert grid.limits == dict(resolution=rc.RESOLUTION, max_x=rc.MAX_XY, max_y=rc.MAX_XY,
                               num_x_cells=nx, num_y_cells=ny)
    np.testing.assert_array_equal(grid.cells != 0, want)


# ---- the host restatement against the reference -------------------------------------------------
def test_cells_on_ray_equals_the_reference_on_every_case(ref, synth):
    out = np.empty((1 << 12, 2), np.int32)
    for r in _all_cases():
        n = ref.ref_ray_to_pixel_mask(r.begin[0], r.begin[1], r.end[0], r.end[1], rc.SCALE, out,
                                      out.shape[0])
        assert 0 < n <= out.shape[0], r.name
        want = {tuple(p) for p in out[:n]}
        got = synth.cells_on_ray(r.begin, r.end, rc.SCALE)
        got_set = {tuple(p) for p in got}
        assert len(want) == n, r.name                              # the reference lists none twice
        assert got_set == want, (r.name, r.begin, r.end)
        assert len(got) == len(got_set), r.name
