"""Device-resident TSDF2D (cartographer_amd/csrc/tsdf_2d.hip): TSDFRangeDataInserter2D::Insert,
ComputeCroppedGrid, the real-time matcher and the fast matcher's stack on the resident planes.

The bar is the one tests/test_gpu_grid.py sets for the probability grid: bit-identical tsd and
weight planes and identical limits after every insert, against tests/golden/tsdf_insert_golden.npz
(made by the reference's own inserter, make_tsdf_insert_golden.py) always, and against the
reference's inserter live (oracle/_ref) wherever it is built.
"""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import make_tsdf_insert_golden as mk  # noqa: E402

GOLDEN_NPZ = os.path.join(GOLDEN, "tsdf_insert_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN_NPZ))


@pytest.fixture(scope="module")
def grid_2d():
    from cartographer_amd import grid_2d as g
    return g


@pytest.fixture(scope="module")
def ref(oracle):
    return oracle if oracle.ref_lib() is not None else None


def _limits_array(lim):
    return np.array([lim["resolution"], lim["max_x"], lim["max_y"], lim["num_x_cells"],
                     lim["num_y_cells"]], np.float64)


def _new_grid(grid_2d, golden, name):
    res, mx, my, nx, ny, t, w = golden[f"{name}/meta"]
    return grid_2d.TSDF2DOnDevice(res, (mx, my), int(nx), int(ny), t, w)


def _num_steps(golden, name):
    return len({k.split("/")[1] for k in golden if k.startswith(name + "/") and
                k.split("/")[1].isdigit()})


def _check_step(dev, golden, name, k, live=None):
    tsd, wgt = dev.planes()
    key = f"{name}/{k}"
    np.testing.assert_array_equal(_limits_array(dev.limits), golden[key + "/limits"],
                                  err_msg=f"{key} limits")
    if key + "/tsd" in golden:
        np.testing.assert_array_equal(tsd, golden[key + "/tsd"], err_msg=f"{key} tsd")
        np.testing.assert_array_equal(wgt, golden[key + "/weight"], err_msg=f"{key} weight")
    if live is not None:
        rt, rw = live.planes()
        assert dev.limits == live.limits, key
        np.testing.assert_array_equal(tsd, rt, err_msg=f"{key} tsd (live reference)")
        np.testing.assert_array_equal(wgt, rw, err_msg=f"{key} weight (live reference)")
    np.testing.assert_array_equal(mk.digest(tsd, wgt), golden[key + "/digest"],
                                  err_msg=f"{key} planes digest")


def _run_scenario(grid_2d, golden, name, ref=None):
    dev = _new_grid(grid_2d, golden, name)
    live = None
    if ref is not None:
        res, mx, my, nx, ny, t, w = golden[f"{name}/meta"]
        live = ref.ReferenceTSDF2D(res, (mx, my), int(nx), int(ny), t, w)
    for k in range(_num_steps(golden, name)):
        origin, returns, opts, repeat = mk.step_inputs(golden, name, k)
        for _ in range(repeat):
            dev.insert(origin, returns, **opts)
            if live is not None:
                live.insert(origin, returns, **opts)
        _check_step(dev, golden, name, k, live)
    return dev


# ---- 1. the eight scenarios of tsdf_range_data_inserter_2d_test.cc -------------------------
REF_SCENARIOS = ["ref_insert_point", "ref_free_space", "ref_linear_weight",
                 "ref_quadratic_weight", "ref_small_angle", "ref_normal_projection",
                 "ref_angle_kernel", "ref_distance_kernel"]


@pytest.mark.parametrize("name", REF_SCENARIOS)
def test_reference_inserter_scenarios_bit_exact(grid_2d, golden, ref, name):
    _run_scenario(grid_2d, golden, name, ref)


def _cell(dev, x, y):
    """(is_known, GetTSD, GetWeight) of the cell holding (x, y) (MapLimits::GetCellIndex)."""
    lim = dev.limits
    ix = int(np.round((lim["max_y"] - y) / lim["resolution"] - 0.5))
    iy = int(np.round((lim["max_x"] - x) / lim["resolution"] - 0.5))
    tsd, wgt = dev.planes()
    t, mw = dev.truncation_distance, dev.max_weight
    if not (0 <= iy < tsd.shape[0] and 0 <= ix < tsd.shape[1]):   # GetTSD outside the limits
        return False, -t, 0.0
    v, w = int(tsd[iy, ix]) & 32767, int(wgt[iy, ix]) & 32767
    scale_t, scale_w = 2 * t / 32766.0, mw / 32766.0
    return (v != 0, -t if v == 0 else v * scale_t + (-t - scale_t),
            0.0 if w == 0 else w * scale_w - scale_w)


@pytest.mark.parametrize("free_space", [False, True])
def test_insert_point_meets_the_reference_tests_expectations(grid_2d, free_space):
    """RangeDataInserterTest2DTSDF.InsertPoint / InsertPointWithFreeSpaceUpdate (:96-203): the
    values and tolerances the reference's test asserts, after one and after 1001 inserts."""
    opts = dict(mk.REF_TEST_OPTIONS, update_free_space=free_space)
    dev = grid_2d.TSDF2DOnDevice(1.0, (1.0, 7.0), 8, 1, 2.0, 10.0)
    dev.insert(mk.ORIGIN, mk.ONE_POINT, **opts)
    t = 2.0
    for y in np.arange(-0.5 if free_space else 1.5, 6.0, 1.0):
        known, tsd, w = _cell(dev, -0.5, y)
        assert known and abs(tsd - max(min(3.5 - y, t), -t)) < 1e-4 and abs(w - 1.0) < 1e-2, y
        for x in (0.5, 1.5):
            known, tsd, w = _cell(dev, x, y)
            assert not known and abs(tsd + t) < 1e-4 and abs(w) < 1e-2
    for _ in range(1000):
        dev.insert(mk.ORIGIN, mk.ONE_POINT, **opts)
    for y in np.arange(-0.5 if free_space else 1.5, 6.0, 1.0):
        known, tsd, w = _cell(dev, -0.5, y)
        assert known and abs(tsd - max(min(3.5 - y, t), -t)) < 1e-4 and abs(w - 10.0) < 1e-2


@pytest.mark.parametrize("exponent,expected", [(1, 1.0 / 4.0), (2, 1.0 / 16.0)])
def test_range_weight_meets_the_reference_tests_expectations(grid_2d, exponent, expected):
    """InsertPointLinearWeight / InsertPointQuadraticWeight (:205-238)."""
    dev = grid_2d.TSDF2DOnDevice(1.0, (1.0, 7.0), 8, 1, 2.0, 10.0)
    dev.insert(mk.ORIGIN, mk.ONE_POINT,
               **dict(mk.REF_TEST_OPTIONS, update_weight_range_exponent=exponent))
    for y in np.arange(1.5, 6.0, 1.0):
        known, tsd, w = _cell(dev, -0.5, y)
        assert known and abs(tsd - max(min(3.5 - y, 2.0), -2.0)) < 1e-4 and abs(w - expected) < 1e-2


# ---- 2. the L-cloud fixture of the real-time matcher test ---------------------------------
def test_l_cloud_fixture_reproduced_from_an_empty_grid(grid_2d):
    """rt2d_tsdf_fixture.npz (make_tsdf_fixture.py: RealTimeCorrelativeScanMatcherTest::SetUpTSDF
    through the reference's own inserter) from an empty 20x20 grid; needs no reference library."""
    f = np.load(os.path.join(GOLDEN, "rt2d_tsdf_fixture.npz"))
    dev = grid_2d.TSDF2DOnDevice(0.05, (0.3, 0.5), 20, 20, 0.3, 1.0)
    dev.insert([0.5, -0.5, 0.0], f["cloud"], truncation_distance=0.3, maximum_weight=10.0,
               update_free_space=False, num_normal_samples=4, sample_radius=0.5,
               project_sdf_distance_to_scan_normal=True, update_weight_range_exponent=0,
               angle_kernel_bandwidth=0.5, distance_kernel_bandwidth=0.5)
    tsd, wgt = dev.planes()
    lim = dev.limits
    assert (lim["resolution"], lim["max_x"], lim["max_y"]) == (
        float(f["resolution"]), float(f["max_x"]), float(f["max_y"]))
    np.testing.assert_array_equal(tsd, f["tsd"])
    np.testing.assert_array_equal(wgt, f["weight"])


# ---- 3. growth and re-updates: twelve room scans, three option sets ------------------------
@pytest.mark.parametrize("name", ["room_lua", "room_free_space", "room_no_kernels"])
def test_room_scans_grow_and_reupdate_bit_exact(grid_2d, golden, ref, name):
    dev = _run_scenario(grid_2d, golden, name, ref)
    assert dev.limits["num_x_cells"] > 16                # the grid grew


# ---- 4. ownership edge cases -----------------------------------------------------------------
def test_ownership_edge_cases_bit_exact(grid_2d, golden, ref):
    """Dense beams with free space, duplicate points, hits inside the truncation distance, an
    angle kernel whose weights underflow to 0 (a later ray takes the cell), an empty insert."""
    _run_scenario(grid_2d, golden, "edges", ref)


def test_angle_kernel_underflow_leaves_cells_to_later_rays(golden):
    """The fixture of the edge cases really exercises the zero-weight rule: the narrow kernel
    step updates cells its lowest-index covering ray could not (weight 0)."""
    before = golden["edges/2/weight"]
    after = golden["edges/3/weight"]
    assert np.count_nonzero(after != before) > 50


def test_created_planes_with_update_markers_are_never_updated(grid_2d, golden):
    """A plane passed to cmx_tsdf2d_create with bit 15 set on a cell: SetCell returns early there
    (tsdf_2d.cc:52-54) and the bit stays; every other cell is what the reference computes."""
    tsd0, wgt0 = golden["edges/0/tsd"], golden["edges/0/weight"]
    res, mx, my, nx, ny, t, w = golden["edges/meta"]
    rng = np.random.default_rng(3)
    marked = (rng.uniform(size=tsd0.shape) < 0.2) & (tsd0 != 0)
    marked |= (rng.uniform(size=tsd0.shape) < 0.02) & (tsd0 == 0)
    start = tsd0.copy()
    start[marked] |= 0x8000
    dev = grid_2d.TSDF2DOnDevice(res, (mx, my), int(nx), int(ny), t, w, start, wgt0)
    origin, returns, opts, _ = mk.step_inputs(golden, "edges", 1)
    dev.insert(origin, returns, **opts)
    tsd, wgt = dev.planes()
    assert dev.limits == dict(resolution=res, max_x=mx, max_y=my, num_x_cells=int(nx),
                              num_y_cells=int(ny))
    np.testing.assert_array_equal(tsd[marked], start[marked])
    np.testing.assert_array_equal(wgt[marked], wgt0[marked])
    np.testing.assert_array_equal(tsd[~marked], golden["edges/1/tsd"][~marked])
    np.testing.assert_array_equal(wgt[~marked], golden["edges/1/weight"][~marked])
    assert np.count_nonzero(golden["edges/1/tsd"][marked] != start[marked] & 0x7fff) > 0


def test_invalid_options_and_range_data(grid_2d):
    from cartographer_amd import _lib
    dev = grid_2d.TSDF2DOnDevice(0.05, (1.0, 1.0), 16, 16, 0.3, 10.0)
    pts = np.array([[0.5, 0.5, 0.0]], np.float32)
    for bad in (dict(num_normal_samples=0), dict(sample_radius=0.0)):
        with pytest.raises(_lib.CmxError) as e:
            dev.insert([0.0, 0.0, 0.0], pts, **dict(mk.LUA_DEFAULTS, **bad))
        assert e.value.status == _lib.INVALID_ARGUMENT
    # z != 0: GrowAsNeeded's box (3D directions) is shorter than the 2D ray end, which lands
    # outside the grown grid: an error, and no cell is written
    far = np.array([[3.5, 0.0, 30.0]], np.float32)
    with pytest.raises(_lib.CmxError) as e:
        dev.insert([0.0, 0.0, 0.0], far, **dict(mk.LUA_DEFAULTS, truncation_distance=0.5))
    assert e.value.status == _lib.INVALID_ARGUMENT
    tsd, wgt = dev.planes()
    assert not tsd.any() and not wgt.any()


# ---- 5. crop ------------------------------------------------------------------------------------
def _crop_restated(oracle, tsd, wgt, t, w):
    """TSDF2D::ComputeCroppedGrid (tsdf_2d.cc:118-135): box of the known cells, each known cell
    written back as SetCell(GetTSD, GetWeight) -- the values round-trip through float."""
    known = tsd != 0
    if not known.any():
        return np.zeros((1, 1), np.uint16), np.zeros((1, 1), np.uint16), (0, 0)
    ys, xs = np.nonzero(known)
    y0, y1, x0, x1 = ys.min(), ys.max(), xs.min(), xs.max()
    ct, cw = tsd[y0:y1 + 1, x0:x1 + 1], wgt[y0:y1 + 1, x0:x1 + 1]
    k = ct != 0
    ref = oracle.ref_lib()

    def to_float(kind, v):
        if ref is not None:
            return ref.ref_tsd_value_to_float(kind, t, w, int(v))
        v = int(v) & 32767
        lo, hi = (-t, t) if kind == 0 else (0.0, w)
        if v == 0:
            return np.float32(lo)
        scale = np.float32((np.float32(hi) - np.float32(lo)) / np.float32(32766.0))
        return np.float32(np.float32(v) * scale + (np.float32(lo) - scale))

    def to_value(kind, x):
        if ref is not None:
            return ref.ref_tsd_float_to_value(kind, t, w, x)
        return oracle.tsd_to_value(x, t) if kind == 0 else oracle.weight_to_value(x, w)

    out_t = np.zeros(ct.shape, np.uint16)
    out_w = np.zeros(cw.shape, np.uint16)
    tmap = {v: to_value(0, to_float(0, v)) for v in np.unique(ct[k])}
    wmap = {v: to_value(1, to_float(1, v)) for v in np.unique(cw[k])}
    out_t[k] = [tmap[v] for v in ct[k]]
    out_w[k] = [wmap[v] for v in cw[k]]
    return out_t, out_w, (x0, y0)


def test_crop_equals_compute_cropped_grid(grid_2d, golden, oracle):
    origin, returns, opts, _ = mk.step_inputs(golden, "room_lua", 0)
    dev = _new_grid(grid_2d, golden, "room_lua")
    dev.insert(origin, returns, **opts)
    tsd, wgt = dev.planes()
    lim = dev.limits
    # some cells with markers from creation and odd weights, so the round trip is not the identity
    tsd = tsd.copy()
    tsd[::9, ::7] |= np.where(tsd[::9, ::7] != 0, 0x8000, 0).astype(np.uint16)
    dev = grid_2d.TSDF2DOnDevice(lim["resolution"], (lim["max_x"], lim["max_y"]),
                                 lim["num_x_cells"], lim["num_y_cells"], 0.3, 10.0, tsd, wgt)
    et, ew, (x0, y0) = _crop_restated(oracle, tsd, wgt, 0.3, 10.0)
    dev.crop()
    ct, cw = dev.planes()
    cl = dev.limits
    assert (cl["num_y_cells"], cl["num_x_cells"]) == et.shape
    assert cl["max_x"] == lim["max_x"] - lim["resolution"] * y0
    assert cl["max_y"] == lim["max_y"] - lim["resolution"] * x0
    np.testing.assert_array_equal(ct, et)
    np.testing.assert_array_equal(cw, ew)
    # a cropped grid takes further inserts like any other
    origin, returns, opts, _ = mk.step_inputs(golden, "room_lua", 1)
    dev.insert(origin, returns, **opts)


def test_crop_of_an_empty_grid(grid_2d):
    dev = grid_2d.TSDF2DOnDevice(0.05, (1.0, 2.0), 16, 8, 0.3, 10.0)
    dev.crop()
    assert dev.limits == dict(resolution=0.05, max_x=1.0, max_y=2.0, num_x_cells=1, num_y_cells=1)
    t, w = dev.planes()
    assert t.shape == (1, 1) and t[0, 0] == 0 and w[0, 0] == 0


# ---- 6. real-time matching on the resident planes -------------------------------------------
def test_resident_real_time_match_equals_host_planes_and_oracle(grid_2d, golden, oracle):
    from cartographer_amd import _lib
    from cartographer_amd import scan_matching as sm
    import ctypes as C
    dev = _new_grid(grid_2d, golden, "room_lua")
    rt = sm.RealTimeCorrelativeScanMatcher2D(0.3, np.deg2rad(8.0), 0.1, 0.1)
    for k in range(4):                                   # the grid version changes between matches
        origin, returns, opts, _ = mk.step_inputs(golden, "room_lua", k)
        dev.insert(origin, returns, **opts)
        scan = returns[::4] - np.array([origin[0], origin[1], 0.0], np.float32)
        init = [float(origin[0]) + 0.07, float(origin[1]) - 0.05, 0.03]
        s_dev, p_dev = rt.match(sm.Rigid2d(*init), scan, dev)
        host = dev.to_host()
        s_host, p_host = rt.match(sm.Rigid2d(*init), scan, host)
        assert s_dev == s_host, k
        assert (p_dev.x, p_dev.y, p_dev.theta) == (p_host.x, p_host.y, p_host.theta), k
        r = oracle.rt2d_match_tsdf(host.cells, host.weight_cells, host.resolution, host.max_x,
                                   host.max_y, 0.3, 10.0, init, scan, 0.3, np.deg2rad(8.0), 0.1,
                                   0.1)
        assert s_dev == r["score"], k
        np.testing.assert_array_equal([p_dev.x, p_dev.y, p_dev.theta], r["pose"])
    # and the direct C entry point with its null checks
    with pytest.raises(_lib.CmxError):
        _lib.check(_lib.lib().cmx_rt2d_match_tsdf_grid(C.byref(rt.options), None, None, None, 0,
                                                       None, None, None))


# ---- 7. the fast matcher's stack from the handle ---------------------------------------------
def test_fast_matcher_from_the_handle(grid_2d, golden, oracle):
    from cartographer_amd import scan_matching as sm
    dev = _new_grid(grid_2d, golden, "room_lua")
    for k in range(6):
        origin, returns, opts, _ = mk.step_inputs(golden, "room_lua", k)
        dev.insert(origin, returns, **opts)
    dev.crop()
    host = dev.to_host()
    depth = 5
    fm_dev = dev.fast_matcher(depth)
    fm_host = sm.FastCorrelativeScanMatcher2D(
        sm.Grid2D(host.cells, host.resolution, host.max_x, host.max_y, -0.3, 0.3), depth)
    ref = oracle.ref_lib()
    for level in range(depth):
        got = fm_dev.level(level)
        np.testing.assert_array_equal(got, fm_host.level(level), err_msg=f"level {level}")
        np.testing.assert_array_equal(got, oracle.precompute2d_range(host.cells, 1 << level,
                                                                     -0.3, 0.3))
        if ref is not None:
            np.testing.assert_array_equal(got, oracle.ref_precompute2d_tsdf(
                host.cells, host.weight_cells, 1 << level, 0.3, 10.0))
    origin, returns, _, _ = mk.step_inputs(golden, "room_lua", 2)
    scan = returns[::3] - np.array([origin[0], origin[1], 0.0], np.float32)
    a = fm_dev.match_full_submap(scan, 0.3)
    b = fm_host.match_full_submap(scan, 0.3)
    assert a[0] == b[0]
    if a[0]:
        assert a[1] == b[1] and (a[2].x, a[2].y, a[2].theta) == (b[2].x, b[2].y, b[2].theta)


# ---- 8. concurrency ---------------------------------------------------------------------------
def test_four_threads_each_with_its_own_grid(grid_2d, golden):
    names = ["room_lua", "room_free_space", "room_no_kernels", "edges"]
    serial = {}
    for name in names:
        dev = _run_scenario(grid_2d, golden, name)
        serial[name] = dev.planes()
    results, errors = {}, []

    def work(name):
        try:
            dev = _new_grid(grid_2d, golden, name)
            for k in range(_num_steps(golden, name)):
                origin, returns, opts, repeat = mk.step_inputs(golden, name, k)
                for _ in range(repeat):
                    dev.insert(origin, returns, **opts)
            results[name] = dev.planes()
        except Exception as e:  # pragma: no cover - reported below
            errors.append((name, e))

    threads = [threading.Thread(target=work, args=(n,)) for n in names]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for name in names:
        np.testing.assert_array_equal(results[name][0], serial[name][0], err_msg=name)
        np.testing.assert_array_equal(results[name][1], serial[name][1], err_msg=name)
