"""The oracle's fast 2D search over a TSDF's cost range against the REFERENCE'S OWN
fast_correlative_scan_matcher_2d.cc over its own TSDF2D (oracle/_ref): found flag equal, f32
score bit-equal, pose to 1e-12.  This pins the expected values of
tests/test_gpu_fast2d_cost_ranges.py; scenes, thresholds and edge cases are those of
tests/fast2d_range_cases.py.

Skipped where neither the reference tree nor a prebuilt oracle/_ref/libref.so exists (the stored
results of tests/golden/fast2d_tsdf_reference.json are checked in test_golden_fast2d_tsdf.py).
"""
import os

import numpy as np
import pytest

import fast2d_range_cases as cases


@pytest.fixture(scope="module")
def ref(oracle):
    lib = oracle.ref_lib()
    if lib is None:
        pytest.skip("reference tree not available and oracle/_ref not prebuilt")
    if not hasattr(lib, "ref_fast2d_create_tsdf") and not os.path.isdir(oracle.REFERENCE):
        pytest.skip("no reference tree, and the prebuilt oracle/_ref predates this entry point")
    return oracle.ReferenceFastCorrelativeScanMatcher2D


def _reference_matcher(ref, sc, tsd, wgt, truncation, depth):
    return ref.over_tsdf(tsd, wgt, cases.RES, sc.max_x, sc.max_y, truncation, cases.MAX_WEIGHT,
                         depth, cases.LIN, cases.ANG)


@pytest.mark.parametrize("truncation", cases.TRUNCATIONS)
@pytest.mark.parametrize("index", range(len(cases.SCENES)))
def test_oracle_equals_the_reference_over_a_tsdf(ref, oracle, synth, index, truncation):
    sc = cases.scene(synth, oracle, index)
    tsd, wgt = sc.planes(truncation)
    assert (tsd == 0).any() and (tsd & 0x8000).any()          # unknown cells and update markers
    rm = _reference_matcher(ref, sc, tsd, wgt, truncation, sc.depth)
    expected, thresholds = cases.tsdf_expectations(synth, oracle, index, truncation)
    assert thresholds[-1] < cases.min_s_of(truncation) <= 1.0 - truncation + 1e-6
    found_at = {t: [] for t in thresholds}
    for (k, full, t), want in expected.items():
        got = cases.run(rm, sc, k, full, t)
        cases.same_result(want, got, (index, truncation, cases.CUTS[k], full, t))
        found_at[t].append(got["found"])
    mid, one, low = thresholds
    assert any(found_at[mid]) and not all(found_at[mid])      # the midpoint separates the clouds
    assert all(found_at[low])
    if truncation == 0.3:
        # a single point on a cell with tsd 0 scores 0.7 + 128 * 0.6 / 255 = 1.00118 > 1
        hits = [r for (k, full, t), r in expected.items() if t == one and r["found"]]
        assert hits and all(r["score"] > 1.0 for r in hits) and not all(found_at[one])


@pytest.mark.parametrize("truncation", cases.TRUNCATIONS + (cases.UNSUPPORTED_TRUNCATION,))
def test_ties_and_floors_equal_the_reference(ref, oracle, synth, truncation):
    """Every candidate at exactly min_s, and a grid with one known cell.  At truncation 1.0 the
    floor is 0.0 (found with score 0.0 for min_score -1); at 1.5 scores are negative: the device
    library refuses that range, and these are the values a lift of the restriction has to meet."""
    sc = cases.scene(synth, oracle, cases.EDGE_SCENE)
    ms = cases.min_s_of(truncation)
    for name, tsd, wgt, init, cloud, min_scores in cases.edge_cases(synth, oracle, truncation):
        om = cases.oracle_matcher(oracle, tsd, sc, sc.depth, -truncation, truncation)
        rm = _reference_matcher(ref, sc, tsd, wgt, truncation, sc.depth)
        for t in min_scores:
            got, want = om.match(init, cloud, t), rm.match(init, cloud, t)
            cases.same_result(got, want, (name, truncation, t))
            if name == "outside":
                assert want["found"] == (t < ms)
                if want["found"]:
                    assert np.float32(want["score"]) == np.float32(ms)
            if name == "one_known" and want["found"]:
                assert ms <= want["score"] < ms + 2.0 * truncation
        if name == "one_known":
            # one of three points on the known cell: above the floor, so found at min_s itself
            assert om.match(init, cloud, ms)["found"]
            assert om.match(init, cloud, ms)["score"] > ms
    if truncation == 1.0:
        name, tsd, wgt, init, cloud, _ = cases.edge_cases(synth, oracle, truncation)[0]
        rm = _reference_matcher(ref, sc, tsd, wgt, truncation, sc.depth)
        r = rm.match(init, cloud, -1.0)
        assert r["found"] and r["score"] == 0.0 and not rm.match(init, cloud, 0.0)["found"]
    if truncation > 1.0:
        name, tsd, wgt, init, cloud, _ = cases.edge_cases(synth, oracle, truncation)[0]
        rm = _reference_matcher(ref, sc, tsd, wgt, truncation, sc.depth)
        r = rm.match(init, cloud, -1.0)
        assert r["found"] and r["score"] == -0.5              # negative: not representable on the device
        # the one-known-cell grid under nine points: one hit, -0.5 + (128 * 3 / 255) / 9 = -0.33268
        name, tsd, wgt, init, _, _ = cases.edge_cases(synth, oracle, truncation)[1]
        om = cases.oracle_matcher(oracle, tsd, sc, sc.depth, -truncation, truncation)
        rm = _reference_matcher(ref, sc, tsd, wgt, truncation, sc.depth)
        want = rm.match(init, cases.LATTICE_CLOUD, -1.0)
        cases.same_result(om.match(init, cases.LATTICE_CLOUD, -1.0), want, (name, "lattice"))
        assert want["found"] and np.float32(want["score"]) == \
            np.float32(-0.5) + np.float32(128.0) * (np.float32(3.0) / np.float32(255.0)) / \
            np.float32(9.0)
        assert -0.34 < want["score"] < -0.33
