"""The fast 2D search on the device over cost ranges other than a probability grid's (a TSDF2D's
tsd plane at truncation distances 0.3, 0.1 and 1.0, one asymmetric range) against the CPU oracle
built with the same range: scores, thresholds, pruning, tie order and the returned pose.

Bars as in tests/test_gpu_2d.py: found flag equal, f32 score bit-equal, pose to 1e-12, integer
work exact.  Expected values always come from the oracle (pinned to the reference's own matcher
over its own TSDF2D by tests/test_reference_ref_fast2d_ranges.py and
tests/golden/fast2d_tsdf_reference.json), never from another device call.  Scenes, clouds and
derived thresholds: tests/fast2d_range_cases.py.
"""
import ctypes as C

import numpy as np
import pytest

import fast2d_range_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sm():
    from cartographer_amd import _lib, scan_matching
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching


def _device_matcher(sm, sc, cells, min_cc, max_cc, depth=None):
    grid = sm.Grid2D(cells, cases.RES, sc.max_x, sc.max_y, min_cc, max_cc)
    return sm.FastCorrelativeScanMatcher2D(grid, depth or sc.depth, cases.LIN, cases.ANG)


def _tsdf_matcher(sm, sc, truncation):
    return _device_matcher(sm, sc, sc.planes(truncation)[0], -truncation, truncation)


def _resident_tsdf_matcher(sm, sc, tsd, wgt, truncation):
    from cartographer_amd import grid_2d
    dev = grid_2d.TSDF2DOnDevice(cases.RES, (sc.max_x, sc.max_y), sc.nx, sc.ny, truncation,
                                 cases.MAX_WEIGHT, tsd, wgt)
    return sm.FastCorrelativeScanMatcher2D.from_device_grid(dev, sc.depth, cases.LIN, cases.ANG)


def _as_result(found, score, pose):
    if not found:
        return dict(found=False)
    return dict(found=True, score=score, pose=[pose.x, pose.y, pose.theta])


def _device_run(sm, gm, init, cloud, min_score):
    if init is None:
        return _as_result(*gm.match_full_submap(cloud, min_score))
    return _as_result(*gm.match(sm.Rigid2d(*init), cloud, min_score))


def _check_scene(sm, oracle, synth, gm, index, truncation):
    sc = cases.scene(synth, oracle, index)
    expected, _ = cases.tsdf_expectations(synth, oracle, index, truncation)
    for (k, full, t), want in expected.items():
        got = _device_run(sm, gm, None if full else sc.inits[k], sc.clouds[k], t)
        cases.same_result(got, want, (index, truncation, cases.CUTS[k], full, t))
    return len(expected)


# ---- a. lowest-resolution sums and scan bounds ------------------------------------------------
@pytest.mark.parametrize("unfused", [0, 1])
@pytest.mark.parametrize("truncation", [0.3, 0.1])
def test_prepare_equals_the_oracle(sm, oracle, synth, debug, truncation, unfused):
    debug(fast2d_unfused=unfused)
    for index in range(len(cases.SCENES)):
        sc = cases.scene(synth, oracle, index)
        om = cases.oracle_tsdf_matcher(synth, oracle, index, truncation)
        gm = _tsdf_matcher(sm, sc, truncation)
        for k, full in cases.searches(sc):
            want = om.prepare([0, 0, 0] if full else sc.inits[k], sc.clouds[k], full)
            got = gm.debug_prepare(None if full else sm.Rigid2d(*sc.inits[k]), sc.clouds[k], full)
            what = str((index, truncation, cases.CUTS[k], full))
            assert got["num_scans"] == want["num_scans"] and got["step"] == want["step"], what
            np.testing.assert_array_equal(got["scans"], want["scans"], err_msg=what)
            np.testing.assert_array_equal(got["bounds"], want["bounds"], err_msg=what)
            np.testing.assert_array_equal(got["sums"], want["sums"], err_msg=what)
            assert want["sums"].size > 0 and want["sums"].max() > 0


# ---- b. single searches -----------------------------------------------------------------------
@pytest.mark.parametrize("truncation", cases.TRUNCATIONS)
@pytest.mark.parametrize("index", range(len(cases.SCENES)))
def test_single_searches_equal_the_oracle(sm, oracle, synth, index, truncation):
    sc = cases.scene(synth, oracle, index)
    assert _check_scene(sm, oracle, synth, _tsdf_matcher(sm, sc, truncation), index,
                        truncation) == 24


@pytest.mark.parametrize("truncation", cases.TRUNCATIONS)
@pytest.mark.parametrize("switches", [
    {"fast2d_queue": 0}, {"fast2d_queue": 2}, {"fast2d_dive": 1},
    {"fast2d_group": 0, "fast2d_group_verify": 1}, {"fast2d_group": 2, "fast2d_group_verify": 1},
    {"fast2d_unfused": 1},
], ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
def test_single_searches_on_every_path(sm, oracle, synth, debug, switches, truncation):
    """The 120 x 120 scene through each search path and front end."""
    debug(**switches)
    sc = cases.scene(synth, oracle, 0)
    _check_scene(sm, oracle, synth, _tsdf_matcher(sm, sc, truncation), 0, truncation)


def test_an_asymmetric_range_equals_the_oracle(sm, oracle, synth):
    """min_correspondence_cost -0.2, max 0.6 over random raw values: min_s = 0.4, max_s = 1.2.
    No reference class produces this range; the oracle (which only reads the two bounds) is the
    expectation."""
    sc = cases.scene(synth, oracle, 2)
    rng = np.random.default_rng(31)
    cells = rng.integers(0, 32768, (sc.ny, sc.nx)).astype(np.uint16)
    cells[rng.random((sc.ny, sc.nx)) < 0.3] = 0
    cells[::5, ::3] |= 0x8000
    om = cases.oracle_matcher(oracle, cells, sc, sc.depth, -0.2, 0.6)
    gm = _device_matcher(sm, sc, cells, -0.2, 0.6)
    for level in range(sc.depth):
        np.testing.assert_array_equal(gm.level(level), om.level(level))
    low = cases.f32(cases.min_s_of(0.6) - 0.05)
    base = {(k, full): cases.run(om, sc, k, full, low) for k, full in cases.searches(sc)}
    thresholds = cases.derive_thresholds([r["score"] for r in base.values()], cases.min_s_of(0.6))
    found = []
    for (k, full) in base:
        for t in thresholds:
            want = cases.run(om, sc, k, full, t)
            got = _device_run(sm, gm, None if full else sc.inits[k], sc.clouds[k], t)
            cases.same_result(got, want, (cases.CUTS[k], full, t))
            found.append(want["found"])
    assert any(found) and not all(found)


# ---- c. ties and floors -----------------------------------------------------------------------
@pytest.mark.parametrize("truncation", [0.3, 1.0])
def test_ties_and_floors_equal_the_oracle(sm, oracle, synth, truncation):
    """Every candidate at exactly min_s (found just below it, in the reference's order among
    thousands of ties; not found at it) and a grid with one known cell.  At truncation 1.0 the
    floor is score 0.0: min_score -1.0 finds it, 0.0 does not."""
    sc = cases.scene(synth, oracle, cases.EDGE_SCENE)
    for name, tsd, _, init, cloud, min_scores in cases.edge_cases(synth, oracle, truncation):
        om = cases.oracle_matcher(oracle, tsd, sc, sc.depth, -truncation, truncation)
        gm = _device_matcher(sm, sc, tsd, -truncation, truncation)
        results = {}
        for t in min_scores:
            want = om.match(init, cloud, t)
            got = _device_run(sm, gm, init, cloud, t)
            cases.same_result(got, want, (name, truncation, t))
            results[t] = want
        if name == "outside":
            ms = cases.min_s_of(truncation)
            assert [r["found"] for r in results.values()][:2] == [True, False]
            assert np.float32(results[min_scores[0]]["score"]) == np.float32(ms)
            if truncation == 1.0:
                assert results[-1.0]["found"] and results[-1.0]["score"] == 0.0
                assert not results[0.0]["found"]


# ---- d. mixed ranges in one launch chain ------------------------------------------------------
def _requantised(score, own, other):
    """The score a search would report for the same level-0 sum if it converted it with another
    problem's (min_s, score_scale)."""
    mean = (np.float32(score) - np.float32(own[0])) / np.float32(own[1])
    return float(np.float32(other[0]) + mean * np.float32(other[1]))


@pytest.fixture(scope="module")
def mixed(sm, oracle, synth):
    """Six matchers of depth 5 over the 120 x 120 scene: probability grid, TSDF 0.3 / 0.1 / 1.0,
    the probability grid again, TSDF 0.3 built from a resident TSDF2D.  Per pair: its range's
    (min_s, score_scale), its oracle matcher, and for both entry points (one cloud for all; a
    cloud per pair) a threshold 0.02 below its own best score (even pairs: found) or above it (odd
    pairs: not found) with the oracle's result at that threshold."""
    sc = cases.scene(synth, oracle, 0)
    lo, hi = sm.K_MIN_CORRESPONDENCE_COST, sm.K_MAX_CORRESPONDENCE_COST
    ranges = [(lo, hi), (-0.3, 0.3), (-0.1, 0.1), (-1.0, 1.0), (lo, hi), (-0.3, 0.3)]
    planes = [sc.cells if r[0] == lo else sc.planes(r[1])[0] for r in ranges]
    device = [_device_matcher(sm, sc, planes[p], *ranges[p]) for p in range(5)]
    device.append(_resident_tsdf_matcher(sm, sc, *sc.planes(0.3), 0.3))
    oracles = [cases.oracle_matcher(oracle, planes[p], sc, sc.depth,
                                    None if ranges[p][0] == lo else ranges[p][0],
                                    None if ranges[p][0] == lo else ranges[p][1])
               for p in range(6)]
    conversion = [(cases.min_s_of(r[1]), cases.score_scale_of(*r)) for r in ranges]
    full = [0, 1, 0, 1, 1, 0]

    def expectations(cloud_of):
        thresholds, want, best = [], [], []
        for p in range(6):
            k = cloud_of(p)
            b = cases.run(oracles[p], sc, k, full[p], cases.f32(conversion[p][0] - 0.05))
            assert b["found"]
            t = cases.f32(b["score"] + (-0.02 if p % 2 == 0 else 0.02))
            r = cases.run(oracles[p], sc, k, full[p], t)
            assert r["found"] == (p % 2 == 0)
            thresholds.append(t)
            want.append(r)
            best.append(b["score"])
        return thresholds, want, best
    return dict(scene=sc, device=device, conversion=conversion, full=full,
                batch=expectations(lambda p: 0), pairs=expectations(lambda p: p % 4))


def _flips_under(conversion, order, thresholds, want, best):
    """Pairs of the call (positions in `order`) that are found, and would not be if their sum
    were converted with the call's problem 0's min_s / score_scale."""
    first = conversion[order[0]]
    return [p for p in order
            if want[p]["found"] and conversion[p] != first and
            not _requantised(best[p], conversion[p], first) > thresholds[p]]


@pytest.mark.parametrize("switches", [{"fast2d_fanout": 0}, {"fast2d_fanout": 1},
                                      {"fast2d_unfused": 1}],
                         ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5), (1, 3, 0, 5, 2, 4)],
                         ids=["in_order", "tsdf_first"])
def test_mixed_ranges_in_one_batch(sm, mixed, debug, order, switches):
    """match_batch and match_pairs over problems of four different ranges: every pair equals its
    own oracle search, so each problem's sums are converted with its own min_s / score_scale.  A
    kernel that took problem 0's conversion for the whole call would lose the pairs named by
    _flips_under (at least one per call)."""
    debug(**switches)
    sc = mixed["scene"]
    matchers = [mixed["device"][p] for p in order]
    full = [mixed["full"][p] for p in order]
    # one cloud for all pairs
    thresholds, want, best = mixed["batch"]
    assert _flips_under(mixed["conversion"], order, thresholds, want, best)
    initial = [sm.Rigid2d(*sc.inits[0])] * 6
    f, s, poses, _ = sm.match_batch(matchers, initial, full, [thresholds[p] for p in order],
                                    sc.clouds[0])
    for i, p in enumerate(order):
        cases.same_result(_as_result(f[i], s[i], poses[i]), want[p], ("match_batch", order, p))
    # a cloud per pair
    thresholds, want, best = mixed["pairs"]
    assert _flips_under(mixed["conversion"], order, thresholds, want, best)
    initial = [sm.Rigid2d(*sc.inits[p % 4]) for p in order]
    f, s, poses, _ = sm.match_pairs(matchers, initial, full, [thresholds[p] for p in order],
                                    [sc.clouds[p % 4] for p in order])
    for i, p in enumerate(order):
        cases.same_result(_as_result(f[i], s[i], poses[i]), want[p], ("match_pairs", order, p))


# ---- e. resident matcher against the golden file ----------------------------------------------
def test_resident_matcher_equals_the_stored_reference_results(sm, oracle, synth):
    """from_device_grid(TSDF2DOnDevice) against the reference's own results, stored."""
    import test_golden_fast2d_tsdf as golden
    import make_fast2d_tsdf_golden as mk
    stored = golden.load()["cases"]
    inputs = mk.selection(cases, synth, oracle)
    assert len(inputs) == len(stored)
    matchers = {}
    for (key, tsd, wgt, truncation, init, cloud, t), entry in zip(inputs, stored):
        assert all(entry[name] == value for name, value in key.items()), (key, entry)
        ident = (key["scene"], truncation, key["kind"])
        if ident not in matchers:
            sc = cases.scene(synth, oracle, key["scene"])
            matchers[ident] = _resident_tsdf_matcher(sm, sc, tsd, wgt, truncation)
        got = _device_run(sm, matchers[ident], init, cloud, t)
        cases.same_result(got, golden.stored_result(entry), key)


# ---- f. sharded -------------------------------------------------------------------------------
def test_sharded_match_over_tsdf_matchers(sm, oracle, synth, debug):
    """cmx_fast2d_match_sharded with the one device as two ranks over TSDF matchers of three
    ranges (submaps 0, 2 and 4 identical): the constraint list equals the oracle's and the
    batch's, and the reduced key names the oracle's best pair -- scores above 1 included."""
    from cartographer_amd import sharding
    debug(comm_virtual_ranks=2)
    comm = sharding.Communicator([0])
    assert comm.num_devices == 2
    sc = cases.scene(synth, oracle, 0)
    truncations = (0.3, 0.1, 0.3, 1.0, 0.3)
    matchers = [_tsdf_matcher(sm, sc, t) for t in truncations]
    full = [1, 1, 0, 1, 1]
    k = 3                                           # the single point: a perfect hit, above 1
    thresholds = [cases.f32(cases.min_s_of(t) - 0.05) for t in truncations]
    want = [cases.run(cases.oracle_tsdf_matcher(synth, oracle, 0, t), sc, k, bool(fl), th)
            for t, fl, th in zip(truncations, full, thresholds)]
    assert all(r["found"] for r in want)
    initial = [sm.Rigid2d(*sc.inits[k])] * 5
    f, s, p, best, _ = comm.match_batch(matchers, initial, full, thresholds, sc.clouds[k])
    f1, s1, p1, _ = sm.match_batch(matchers, initial, full, thresholds, sc.clouds[k])
    for i in range(5):
        cases.same_result(_as_result(f[i], s[i], p[i]), want[i], ("sharded", i))
        cases.same_result(_as_result(f1[i], s1[i], p1[i]), want[i], ("batch", i))
    scores = np.array([r["score"] for r in want], np.float32)
    assert best[0] == int(np.argmax(scores)) == int(np.argmax(s1))      # first maximum
    assert np.float32(best[1]) == scores[best[0]] and scores[best[0]] > 1.0
    assert s[0] == s[4]


# ---- ranges the search cannot represent -------------------------------------------------------
def test_a_range_with_negative_scores_is_refused(sm, oracle, synth):
    """max_correspondence_cost > 1 gives scores down to 1 - max_correspondence_cost < 0, which
    the search (scores ordered by their bit patterns, negative = no candidate) cannot hold: every
    creation call that can receive such a range answers CMX_INVALID_ARGUMENT and says why.  (A
    resident probability grid always has the probability range; its call keeps creating.)"""
    from cartographer_amd import _lib, grid_2d
    sc = cases.scene(synth, oracle, cases.EDGE_SCENE)
    t = cases.UNSUPPORTED_TRUNCATION
    tsd, wgt = sc.planes(1.0)
    with pytest.raises(_lib.CmxError) as e:
        _device_matcher(sm, sc, tsd, -t, t)
    assert e.value.status == _lib.INVALID_ARGUMENT and "negative" in str(e.value)
    with pytest.raises(_lib.CmxError) as e:
        _device_matcher(sm, sc, tsd, 0.0, float(np.nextafter(np.float32(1.0), np.float32(2.0))))
    assert e.value.status == _lib.INVALID_ARGUMENT and "negative" in str(e.value)
    with pytest.raises(_lib.CmxError) as e:
        _resident_tsdf_matcher(sm, sc, tsd, wgt, t)
    assert e.value.status == _lib.INVALID_ARGUMENT and "negative" in str(e.value)
    h = C.c_void_p()
    dev = grid_2d.TSDF2DOnDevice(cases.RES, (sc.max_x, sc.max_y), sc.nx, sc.ny, t,
                                 cases.MAX_WEIGHT, tsd, wgt)
    options = _lib.Fast2DOptions(cases.LIN, cases.ANG, sc.depth)
    assert _lib.lib().cmx_fast2d_create_from_tsdf(C.byref(options), dev._h, C.byref(h)) == \
        _lib.INVALID_ARGUMENT
    assert not h
    # what stays supported: the default range (host cells and a resident grid), T = 0.3, T = 1.0
    _device_matcher(sm, sc, sc.cells, sm.K_MIN_CORRESPONDENCE_COST, sm.K_MAX_CORRESPONDENCE_COST)
    pg = grid_2d.ProbabilityGridOnDevice(cases.RES, (sc.max_x, sc.max_y), sc.nx, sc.ny, sc.cells)
    sm.FastCorrelativeScanMatcher2D.from_device_grid(pg, sc.depth, cases.LIN, cases.ANG)
    _resident_tsdf_matcher(sm, sc, *sc.planes(0.3), 0.3)
    _resident_tsdf_matcher(sm, sc, tsd, wgt, 1.0)
