"""tests/golden/fast2d_tsdf_reference.json (CPU): the reference's stored fast 2D results over
TSDF2Ds are what the oracle computes, with or without oracle/_ref, and the file regenerates
identically wherever oracle/_ref builds."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)


def load():
    with open(os.path.join(GOLDEN, "fast2d_tsdf_reference.json")) as f:
        return json.load(f)


def stored_result(entry):
    if not entry["found"]:
        return dict(found=False)
    return dict(found=True, score=float.fromhex(entry["score"]),
                pose=np.array([float.fromhex(v) for v in entry["pose"]]))


def test_oracle_reproduces_the_stored_reference_results(oracle, synth):
    import fast2d_range_cases as cases
    import make_fast2d_tsdf_golden as mk
    stored = load()
    inputs = mk.selection(cases, synth, oracle)
    assert len(inputs) == len(stored["cases"]) >= 40
    kinds = set()
    for (key, tsd, _, truncation, init, cloud, t), entry in zip(inputs, stored["cases"]):
        assert all(entry[name] == value for name, value in key.items()), (key, entry)
        sc = cases.scene(synth, oracle, key["scene"])
        om = cases.oracle_matcher(oracle, tsd, sc, sc.depth, -truncation, truncation)
        got = om.match_full_submap(cloud, t) if init is None else om.match(init, cloud, t)
        cases.same_result(got, stored_result(entry), key)
        kinds.add((key["kind"], entry["found"]))
    # found and not found, in the scenes and in both edge cases
    assert kinds == {(k, f) for k in ("scene", "outside", "one_known") for f in (False, True)}


def test_golden_regenerates_identically(oracle):
    lib = oracle.ref_lib()
    if lib is None:
        pytest.skip("reference tree not available and oracle/_ref not prebuilt")
    if not hasattr(lib, "ref_fast2d_create_tsdf") and not os.path.isdir(oracle.REFERENCE):
        pytest.skip("no reference tree, and the prebuilt oracle/_ref predates this entry point")
    import make_fast2d_tsdf_golden as mk
    assert mk.build() == load()
