"""Batched real-time matching on resident TSDF2Ds (cartographer_amd/csrc/rt_2d_tsdf.hip):
cmx_rt2d_match_tsdf_grid_batch and cmx_rt2d_match_tsdf_grid_batch_resident.

Every comparison is `==` on the score and assert_array_equal on the pose: against the oracle's
restatement (oracle.rt2d_match_tsdf) always, and against the reference's own matcher
(oracle.ref_rt2d_match) wherever oracle/_ref is built.

The entries route every batch size to the per-candidate batch kernels (the bulk path measured
slower); the tests run the integer bulk path under the debug switch
rt2d_tsdf_batch_bulk and assert from the statistics that it is that path they saw.
"""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
for p in (GOLDEN, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_tsdf_insert_golden as mk  # noqa: E402
import tsdf_helpers  # noqa: E402

T, W = 0.3, 10.0                      # the TSDValueConverter of every grid here
ANG, TW, RW = float(np.deg2rad(8.0)), 0.1, 0.1
# Linear windows at 5 cm cells: nl = 0, 2, 6 and 7, the largest the bulk kernel takes.
WINDOWS = (0.0, 0.1, 0.3, 0.35)
FINALIST_CAPACITY = 4096              # rt_2d_device.h kFinalistCap: the list a match may overflow
# Candidates reach that list when their exact weighted score is within 1e-5 of the best (the
# survivors of the integer intervals have a slot each and cannot overflow); ten times that.
INTERVAL_WIDTH = 1e-4


class Triple:
    def __init__(self, grid, host, scan, init):
        self.grid, self.host, self.scan, self.init = grid, host, scan, init


def _oracle_match(oracle, tr, lin, want_scores=False):
    h = tr.host
    return oracle.rt2d_match_tsdf(h.cells, h.weight_cells, h.resolution, h.max_x, h.max_y,
                                  h.truncation_distance, h.max_weight, tr.init, tr.scan, lin, ANG,
                                  TW, RW, want_scores=want_scores)


def _check(oracle, tr, lin, score, pose, label):
    r = _oracle_match(oracle, tr, lin)
    assert score == r["score"], label
    np.testing.assert_array_equal(np.asarray(pose, np.float64), r["pose"], err_msg=str(label))
    if oracle.ref_lib() is not None:
        h = tr.host
        ref = oracle.ref_rt2d_match(h.cells, h.resolution, h.max_x, h.max_y, tr.init, tr.scan,
                                    lin, ANG, TW, RW, weight_cells=h.weight_cells,
                                    truncation_distance=h.truncation_distance,
                                    max_weight=h.max_weight)
        assert score == ref["score"], label
        np.testing.assert_array_equal(np.asarray(pose, np.float64), ref["pose"],
                                      err_msg=str(label))


def _matcher(sm, lin):
    return sm.RealTimeCorrelativeScanMatcher2D(lin, ANG, TW, RW)


def _run(sm, lin, triples):
    scores, poses, stats = sm.rt2d_match_batch(
        _matcher(sm, lin), [t.grid for t in triples], [sm.Rigid2d(*t.init) for t in triples],
        [t.scan for t in triples])
    return scores, [[p.x, p.y, p.theta] for p in poses], stats


def _room_triples(grid_2d, golden, name, counts):
    """A grid grown scan by scan from the golden steps; after every third insert a match of a
    later step's scan against a copy of the planes as they are then."""
    res, mx, my, nx, ny, t, w = golden[f"{name}/meta"]
    dev = grid_2d.TSDF2DOnDevice(res, (mx, my), int(nx), int(ny), t, w)
    out = []
    for k in range(12):
        origin, returns, opts, _ = mk.step_inputs(golden, name, k)
        dev.insert(origin, returns, **opts)
        if k % 3 != 2:
            continue
        host = dev.to_host()
        grid = grid_2d.TSDF2DOnDevice(res, (host.max_x, host.max_y), host.cells.shape[1],
                                      host.cells.shape[0], t, w, host.cells, host.weight_cells)
        for j, count in enumerate(counts):
            o, r, _, _ = mk.step_inputs(golden, name, (k + j) % 12)
            scan = (r - np.array([o[0], o[1], 0.0], np.float32))[:: max(1, len(r) // count)][:count]
            init = [float(o[0]) + 0.04 - 0.02 * j, float(o[1]) - 0.03 + 0.015 * j, 0.02 - 0.01 * j]
            out.append(Triple(grid, host, np.ascontiguousarray(scan), init))
    return out


def _synth_triples(grid_2d, sm, oracle, synth, seed, nx, ny, counts):
    cells, lim, world = synth.make_submap(seed, nx, ny, 0.05, 20, 600, 5.0, 0.01)
    tsd, wgt = tsdf_helpers.tsdf_from_probability_grid(oracle, cells, 0.05, T, W, seed)
    host = sm.TSDF2D(tsd, wgt, 0.05, lim["max_x"], lim["max_y"], T, W)
    grid = grid_2d.TSDF2DOnDevice(0.05, (lim["max_x"], lim["max_y"]), nx, ny, T, W, tsd, wgt)
    out = []
    for j, count in enumerate(counts):
        pose = world.free_pose(seed * 100 + j, 0.5)
        scan = world.scan(pose, count, 5.0, 0.01, j)
        init = [pose[0] + 0.06 - 0.01 * j, pose[1] - 0.04, pose[2] + 0.02]
        out.append(Triple(grid, host, scan, init))
    return out, (cells, lim, world)


@pytest.fixture(autouse=True)
def bulk_path(debug):
    debug(rt2d_tsdf_batch_bulk=1)
    yield


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "tsdf_insert_golden.npz")))


@pytest.fixture(scope="module")
def grid_2d():
    from cartographer_amd import grid_2d as g
    return g


@pytest.fixture(scope="module")
def sm():
    from cartographer_amd import scan_matching
    return scan_matching


@pytest.fixture(scope="module")
def triples(grid_2d, sm, oracle, synth, golden):
    """132 distinct (grid, scan, pose) triples: grids grown by insert from the golden room steps
    (lua defaults and free space), grids with random weights, an unknown band and update markers;
    a non-square grid and one that needs more than one LDS tile; 1 to over 1000 points."""
    out = []
    out += _room_triples(grid_2d, golden, "room_lua", (997, 333, 130, 61, 250, 501, 17, 777))
    out += _room_triples(grid_2d, golden, "room_free_space", (1000, 65, 499, 203, 37, 640, 1, 90))
    out += _synth_triples(grid_2d, sm, oracle, synth, 11, 200, 200,
                          [1300, 63, 129, 1001, 450, 7, 300, 911, 222, 575, 35, 705, 150, 843, 95,
                           1025, 401, 260, 3, 666, 519, 188, 1280, 77])[0]
    out += _synth_triples(grid_2d, sm, oracle, synth, 12, 150, 230,
                          [333, 1003, 97, 610, 41, 870, 205, 511, 739, 123, 999, 58, 286, 447, 1060,
                           161, 690, 19, 375, 820, 550, 253])[0]
    out += _synth_triples(grid_2d, sm, oracle, synth, 13, 360, 330,
                          [1013, 301, 87, 655, 143, 907, 470, 29, 761, 233, 1290, 395, 566, 171,
                           833, 69, 949, 317, 620, 111, 1031, 483])[0]
    assert len(out) >= 128
    return out


def test_parity_on_distinct_triples_through_the_bulk_path(sm, oracle, triples):
    """Every triple under one of four windows (nl = 0 ... 7): score and pose equal the oracle's
    (and the reference's own) bit for bit, and the statistics show the bulk path at work: the
    candidates weighted on the host are a small share of the search space, which a call that had
    fallen back to the per-candidate kernels (every candidate a finalist) cannot show."""
    assert len({(id(t.grid), t.scan.tobytes(), tuple(t.init)) for t in triples}) >= 128
    assert min(len(t.scan) for t in triples) == 1 and max(len(t.scan) for t in triples) > 1000
    assert any(len(t.scan) % 64 for t in triples)
    shapes = {t.host.cells.shape for t in triples}
    assert any(s[0] != s[1] for s in shapes) and any(s[0] * s[1] > 100000 for s in shapes)
    for w, lin in enumerate(WINDOWS):
        part = triples[w::len(WINDOWS)]
        # Precondition, on the oracle's own landscape: the best score is positive and the
        # candidates within the interval width of the best are far below the list capacity.
        total = 0
        for k, tr in enumerate(part):
            r = _oracle_match(oracle, tr, lin, want_scores=True)
            best = float(r["scores"].max())
            assert best > 0.0, (lin, k)
            near = int(np.count_nonzero(r["scores"] >= best * (1.0 - INTERVAL_WIDTH)))
            assert near < FINALIST_CAPACITY // 8, (lin, k, near, r["num_candidates"])
            total += r["num_candidates"]
        scores, poses, stats = _run(sm, lin, part)
        print(f"window {lin}: {len(part)} matches, stats {stats}")
        for k, tr in enumerate(part):
            _check(oracle, tr, lin, scores[k], poses[k], (lin, k))
        assert stats["candidates_scored"] == total
        assert stats["coarse_candidates"] == total
        if lin > 0.0:   # (nl = 0: a handful of candidates per match, all of them near the best)
            assert stats["finalists"] * 20 < stats["candidates_scored"], stats
            assert stats["refined_candidates"] < stats["candidates_scored"], stats


def test_partner_equality(sm, oracle, triples, debug):
    """The same batch with the legacy switch set (one thread per candidate) returns bitwise-equal
    scores and poses."""
    part = triples[::2]
    a_scores, a_poses, a_stats = _run(sm, 0.3, part)
    debug(rt2d_tsdf_batch_legacy=1)
    b_scores, b_poses, b_stats = _run(sm, 0.3, part)
    np.testing.assert_array_equal(np.array(a_scores), np.array(b_scores))
    np.testing.assert_array_equal(np.array(a_poses), np.array(b_poses))
    assert b_stats["finalists"] == b_stats["candidates_scored"]      # the per-candidate path
    assert a_stats["finalists"] * 20 < a_stats["candidates_scored"]


def test_default_routing_is_the_per_candidate_batch(sm, oracle, triples):
    """Without a switch the entries run the per-candidate batch kernels (every candidate a
    finalist) and return the same bits."""
    from cartographer_amd import _lib
    part = triples[3::9]
    a_scores, a_poses, _ = _run(sm, 0.3, part)
    _lib.debug_reset()
    b_scores, b_poses, b_stats = _run(sm, 0.3, part)
    np.testing.assert_array_equal(np.array(a_scores), np.array(b_scores))
    np.testing.assert_array_equal(np.array(a_poses), np.array(b_poses))
    assert b_stats["finalists"] == b_stats["candidates_scored"]


def test_verify_switch(sm, oracle, triples, debug):
    """Every candidate's exact score lies in its interval (checked on the device for the whole
    search space; the call fails otherwise)."""
    debug(rt2d_tsdf_verify=1, rt2d_tsdf_batch_bulk=1)
    for lin in (0.1, 0.35):
        part = triples[::5]
        scores, poses, stats = _run(sm, lin, part)
        # the bulk path ran (on the per-candidate path, which has no intervals to check, every
        # candidate is a finalist)
        assert stats["finalists"] * 20 < stats["candidates_scored"], stats
        for k, tr in enumerate(part[:6]):
            _check(oracle, tr, lin, scores[k], poses[k], (lin, k))


def test_degenerate_matches_mixed_into_a_normal_batch(sm, grid_2d, oracle, triples):
    """An all-unknown TSDF (score 0 everywhere: the first candidate wins), a scan wholly outside
    the grid, a one-point cloud and a grid with known tsd and zero weights among normal matches:
    every result is the oracle's, and only the flat matches are repeated on the per-candidate
    kernels."""
    normal = [t for t in triples if t.host.cells.shape == (200, 200) and len(t.scan) > 200][:12]
    base = normal[0]
    h = base.host
    zeros = np.zeros_like(h.cells)

    def variant(tsd, wgt, scan, init):
        host = sm.TSDF2D(tsd, wgt, h.resolution, h.max_x, h.max_y, T, W)
        grid = grid_2d.TSDF2DOnDevice(h.resolution, (h.max_x, h.max_y), tsd.shape[1],
                                      tsd.shape[0], T, W, tsd, wgt)
        return Triple(grid, host, scan, init)

    zero_weight = np.where((h.weight_cells & 32767) > 0, 1, 0).astype(np.uint16)   # value 1: weight 0
    flat = [variant(zeros, zeros, base.scan, base.init),
            Triple(base.grid, base.host, base.scan,
                   [h.max_x + 40.0, h.max_y + 40.0, 0.3]),
            variant(h.cells, zero_weight, base.scan, base.init)]
    one_point = Triple(base.grid, base.host, base.scan[100:101].copy(), base.init)
    batch = normal[:4] + [flat[0]] + normal[4:8] + [flat[1], one_point] + normal[8:] + [flat[2]]
    scores, poses, stats = _run(sm, 0.3, batch)
    refs = [_oracle_match(oracle, tr, 0.3) for tr in batch]
    for k, tr in enumerate(batch):
        _check(oracle, tr, 0.3, scores[k], poses[k], k)
    for tr in flat:                                  # score 0 everywhere: the first candidate
        r = _oracle_match(oracle, tr, 0.3)
        assert r["score"] == 0.0
    per_match = refs[0]["num_candidates"]
    flat_total = sum(_oracle_match(oracle, tr, 0.3)["num_candidates"] for tr in flat)
    # (the three flat matches scored every candidate with the f32 chains, the others a few)
    assert flat_total <= stats["finalists"] < flat_total + (len(batch) - 3) * per_match // 20, stats
    assert stats["candidates_scored"] == sum(r["num_candidates"] for r in refs)


def test_grid_version_rebuilds_the_images(sm, grid_2d, oracle, golden):
    """A batch, an insert into some of its grids, the batch again: the results equal the oracle
    on the new planes."""
    res, mx, my, nx, ny, t, w = golden["room_lua/meta"]
    grids = [grid_2d.TSDF2DOnDevice(res, (mx, my), int(nx), int(ny), t, w) for _ in range(4)]
    for g in grids:
        for k in range(5):
            origin, returns, opts, _ = mk.step_inputs(golden, "room_lua", k)
            g.insert(origin, returns, **opts)
    o, r, _, _ = mk.step_inputs(golden, "room_lua", 5)
    scan = np.ascontiguousarray((r - np.array([o[0], o[1], 0.0], np.float32))[::2])
    init = [float(o[0]) + 0.05, float(o[1]) - 0.04, 0.02]
    batch = sm.Rt2DBatch(_matcher(sm, 0.3), grids, [scan] * 4)
    inits = np.array([init] * 4)
    for round_ in range(3):
        scores, poses, _ = batch.match(inits)
        for k, g in enumerate(grids):
            _check(oracle, Triple(g, g.to_host(), scan, init), 0.3, scores[k], poses[k],
                   (round_, k))
        for k in (0, 2):                              # grids 1 and 3 keep their version
            origin, returns, opts, _ = mk.step_inputs(golden, "room_lua", 5 + round_ + k)
            grids[k].insert(origin, returns, **opts)


def test_resident_clouds_and_a_batch_of_one(sm, oracle, triples):
    part = triples[2::11]
    lin = 0.3
    host_scores, host_poses, _ = _run(sm, lin, part)
    batch = sm.Rt2DBatch(_matcher(sm, lin), [t.grid for t in part], [t.scan for t in part],
                         resident=True)
    scores, poses, stats = batch.match(np.array([t.init for t in part]))
    np.testing.assert_array_equal(scores, np.array(host_scores))
    np.testing.assert_array_equal(poses, np.array(host_poses))
    assert stats["finalists"] * 20 < stats["candidates_scored"]
    rt = _matcher(sm, lin)
    for k, tr in enumerate(part[:4]):
        s1, p1, _ = _run(sm, lin, [tr])
        s, p = rt.match(sm.Rigid2d(*tr.init), tr.scan, tr.grid)
        assert s1[0] == s == host_scores[k]
        np.testing.assert_array_equal(p1[0], [p.x, p.y, p.theta])
        np.testing.assert_array_equal(p1[0], host_poses[k])


def test_four_host_threads(sm, grid_2d, oracle, triples):
    """Four threads, each with grids and batches of its own, concurrently: all results exact."""
    lin = 0.3
    parts = []
    for i in range(4):
        own = []
        for tr in triples[i::16]:
            h = tr.host
            grid = grid_2d.TSDF2DOnDevice(h.resolution, (h.max_x, h.max_y), h.cells.shape[1],
                                          h.cells.shape[0], T, W, h.cells, h.weight_cells)
            own.append(Triple(grid, h, tr.scan, tr.init))
        parts.append(own)
    refs = [[_oracle_match(oracle, tr, lin) for tr in part] for part in parts]
    errors = []

    def work(i):
        try:
            for _ in range(5):
                scores, poses, _ = _run(sm, lin, parts[i])
                for k, r in enumerate(refs[i]):
                    assert scores[k] == r["score"], (i, k)
                    np.testing.assert_array_equal(np.asarray(poses[k]), r["pose"])
        except BaseException as e:   # noqa: BLE001 - reported on the main thread
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_two_threads_batch_on_the_same_grids(sm, grid_2d, oracle, golden):
    """Two threads batch at once on the same grids, each grid twice in a batch, with an insert
    into some grids between the rounds: whichever thread finds a grid's images being built (or
    stale while the other still reads them) builds its own for the call, and every result is the
    oracle's on the planes of that round."""
    res, mx, my, nx, ny, t, w = golden["room_lua/meta"]
    grids = [grid_2d.TSDF2DOnDevice(res, (mx, my), int(nx), int(ny), t, w) for _ in range(3)]
    for g in grids:
        for k in range(4):
            origin, returns, opts, _ = mk.step_inputs(golden, "room_lua", k)
            g.insert(origin, returns, **opts)
    lin = 0.3
    items = []
    for j in range(6):                                 # grids 0 1 2 0 1 2
        o, r, _, _ = mk.step_inputs(golden, "room_lua", 4 + j)
        scan = np.ascontiguousarray((r - np.array([o[0], o[1], 0.0], np.float32))[j % 2::3])
        items.append((grids[j % 3], scan, [float(o[0]) + 0.03, float(o[1]) - 0.02, 0.01 * j]))
    for round_ in range(3):
        hosts = [g.to_host() for g in grids]
        part = [Triple(g, hosts[j % 3], scan, init) for j, (g, scan, init) in enumerate(items)]
        refs = [_oracle_match(oracle, tr, lin) for tr in part]
        barrier = threading.Barrier(2)
        errors = []

        def work(i):
            try:
                barrier.wait()
                for _ in range(3):
                    scores, poses, stats = _run(sm, lin, part)
                    assert stats["finalists"] * 20 < stats["candidates_scored"], stats
                    for k, r in enumerate(refs):
                        assert scores[k] == r["score"], (round_, i, k)
                        np.testing.assert_array_equal(np.asarray(poses[k]), r["pose"])
            except BaseException as e:   # noqa: BLE001 - reported on the main thread
                errors.append((round_, i, repr(e)))

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for k in (0, 2):                               # grid 1 keeps its version
            origin, returns, opts, _ = mk.step_inputs(golden, "room_lua", 8 + round_ + k // 2)
            grids[k].insert(origin, returns, **opts)


def test_a_grid_wider_than_one_tile(sm, grid_2d, oracle, triples):
    """The planes of a 200 x 200 grid set into unknown planes of 260 x 1150 cells, across the
    column where the sum kernel's first LDS tile ends (a tile's core holds 1024 image columns):
    the kernel walks tiles in x and in y, and both tiles in x hold known cells."""
    src = [t for t in triples if t.host.cells.shape == (200, 200) and len(t.scan) > 60][:8]
    row0, col0, ny, nx = 30, 905, 260, 1150
    wide = {}
    out = []
    for tr in src:
        if id(tr.host) not in wide:
            h = tr.host
            tsd, wgt = np.zeros((ny, nx), np.uint16), np.zeros((ny, nx), np.uint16)
            tsd[row0:row0 + 200, col0:col0 + 200] = h.cells
            wgt[row0:row0 + 200, col0:col0 + 200] = h.weight_cells
            # rows count down from max_x and columns from max_y (MapLimits::GetCellIndex)
            max_x, max_y = h.max_x + row0 * h.resolution, h.max_y + col0 * h.resolution
            wide[id(tr.host)] = (
                sm.TSDF2D(tsd, wgt, h.resolution, max_x, max_y, T, W),
                grid_2d.TSDF2DOnDevice(h.resolution, (max_x, max_y), nx, ny, T, W, tsd, wgt))
        host, grid = wide[id(tr.host)]
        out.append(Triple(grid, host, tr.scan, tr.init))
    for lin in (0.3, 0.35):
        for k, tr in enumerate(out):
            r = _oracle_match(oracle, tr, lin, want_scores=True)
            best = float(r["scores"].max())
            assert best > 0.0, (lin, k)
            near = int(np.count_nonzero(r["scores"] >= best * (1.0 - INTERVAL_WIDTH)))
            assert near < FINALIST_CAPACITY // 8, (lin, k, near)
            # the match's known cells lie on both sides of the tile boundary
            known = np.nonzero((tr.host.weight_cells & 32767).any(axis=0))[0]
            assert known.min() < 1000 < 1030 < known.max()
        scores, poses, stats = _run(sm, lin, out)
        for k, tr in enumerate(out):
            _check(oracle, tr, lin, scores[k], poses[k], (lin, k))
        assert stats["finalists"] * 20 < stats["candidates_scored"], stats


def test_argument_checks(sm, grid_2d, synth, triples):
    from cartographer_amd import _lib
    tr = triples[0]
    cells, lim, _ = synth.make_submap(5, 64, 64, 0.05, 4, 100, 5.0, 0.01)
    prob = grid_2d.ProbabilityGridOnDevice(0.05, (lim["max_x"], lim["max_y"]), 64, 64, cells=cells)
    with pytest.raises(ValueError):
        sm.rt2d_match_batch(_matcher(sm, 0.3), [tr.grid, prob], [sm.Rigid2d(*tr.init)] * 2,
                            [tr.scan] * 2)
    with pytest.raises(ValueError):
        sm.Rt2DBatch(_matcher(sm, 0.3), [prob, tr.grid], [tr.scan] * 2, resident=True)
    L = _lib.lib()
    opts = _matcher(sm, 0.3).options
    assert L.cmx_rt2d_match_tsdf_grid_batch(C.byref(opts), None, 1, None, None, None, None, None,
                                            None) == _lib.INVALID_ARGUMENT
    handles = (C.c_void_p * 1)(tr.grid._h)
    assert L.cmx_rt2d_match_tsdf_grid_batch(C.byref(opts), handles, 0, None, None, None, None,
                                            None, None) == _lib.INVALID_ARGUMENT


def test_grids_on_two_devices_are_rejected(sm, grid_2d, triples):
    from cartographer_amd import _lib
    if _lib.lib().cmx_device_count() < 2:
        pytest.skip("one HIP device")
    tr = triples[0]
    h = tr.host
    other = grid_2d.TSDF2DOnDevice(h.resolution, (h.max_x, h.max_y), h.cells.shape[1],
                                   h.cells.shape[0], T, W, h.cells, h.weight_cells, device=1)
    with pytest.raises(_lib.CmxError):
        sm.rt2d_match_batch(_matcher(sm, 0.3), [tr.grid, other], [sm.Rigid2d(*tr.init)] * 2,
                            [tr.scan] * 2)
