"""Loop closure over 3D submaps resident in HBM: the reference's ConstraintBuilder3D, unmodified,
over submaps that ActiveSubmaps3D filled from simulated sweeps
(examples/dropin/constraint_builder_3d_submaps_main.cc), built four ways -- the reference's own
submaps, inserter and matchers (the golden), our adapters over host grids, resident submaps whose
fast matchers come from cmx_fast3d_create_from_grids, and the same under the batched builder."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "examples", "dropin")
DROPIN_BUILD = os.path.join(ROOT, "oracle", "_ref", "dropin")
REFERENCE = "/root/reference"
NAME = "constraint_builder_3d_submaps"
BUILDS = {k: os.path.join(DROPIN_BUILD, f"{NAME}_{k}")
          for k in ("reference", "mi355x", "resident_mi355x", "batched_resident_mi355x")}
GOLDEN = os.path.join(ROOT, "tests", "golden", f"{NAME}_reference.txt")


def _constraints(text):
    """{(submap, node, tag): sorted list of [t xyz, q wxyz]} of the constraint lines (a node's
    local and global constraint to one submap share the key), and the count line."""
    out, count = {}, None
    for line in text.splitlines():
        w = line.split()
        if line.startswith("constraint submap"):
            key = (int(w[2]), int(w[4]), int(w[15]))
            out.setdefault(key, []).append([float(v) for v in w[6:9] + w[10:14]])
        elif line.startswith("constraints"):
            count = int(w[1])
    return {k: sorted(v) for k, v in out.items()}, count


def test_golden_has_local_and_global_constraints_over_three_submaps():
    text = open(GOLDEN).read()
    assert "finished submaps 3" in text
    got, count = _constraints(text)
    assert count == sum(len(v) for v in got.values()) >= 4
    assert len({k[0] for k in got}) == 3                # every submap closes a loop


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree to compile")
def test_builds_exist_and_resident_ones_link_the_device_constructor():
    subprocess.run(["make", "-C", DROPIN, f"OUT={DROPIN_BUILD}"] + list(BUILDS.values()),
                   check=True, capture_output=True)
    for path in BUILDS.values():
        assert os.path.exists(path), path
    for key in ("resident_mi355x", "batched_resident_mi355x"):
        symbols = subprocess.run(["nm", "-C", BUILDS[key]], check=True, capture_output=True,
                                 text=True).stdout
        assert "cmx_fast3d_create_from_grids" in symbols
        assert "cmx_grid3d_insert" in symbols
        assert "RangeDataInserter3D::Insert" not in symbols
    symbols = subprocess.run(["nm", "-C", BUILDS["mi355x"]], check=True, capture_output=True,
                             text=True).stdout
    assert "RangeDataInserter3D::Insert" in symbols and "cmx_fast3d_create" in symbols


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree to compile")
def test_reference_build_reproduces_its_golden():
    subprocess.run(["make", "-C", DROPIN, f"OUT={DROPIN_BUILD}", BUILDS["reference"]], check=True,
                   capture_output=True)
    out = subprocess.run([BUILDS["reference"]], check=True, capture_output=True,
                         timeout=120).stdout
    assert out == open(GOLDEN, "rb").read()


@pytest.mark.gpu
def test_device_builds_agree_with_each_other_and_the_golden():
    """The adapter, resident and batched-resident builds run to completion (before the resident
    constructor existed, the resident build aborted in Flatten), print byte-identical constraint
    lines, and those match the golden: same (submap, node, tag) set, transforms within 1e-6."""
    lines = {}
    for key in ("mi355x", "resident_mi355x", "batched_resident_mi355x"):
        path = BUILDS[key]
        assert os.path.exists(path), "oracle/_ref/dropin is prebuilt by __graft_entry__.build()"
        run = subprocess.run([path], check=True, capture_output=True, text=True, timeout=300)
        lines[key] = [l for l in run.stdout.splitlines() if l.startswith("constraint")]
    assert lines["resident_mi355x"] == lines["mi355x"]
    assert lines["batched_resident_mi355x"] == lines["mi355x"]
    got, count = _constraints("\n".join(lines["mi355x"]))
    want, want_count = _constraints(open(GOLDEN).read())
    assert count == sum(len(v) for v in got.values())
    assert want_count == sum(len(v) for v in want.values())
    assert set(got) == set(want)
    for key in want:
        assert len(got[key]) == len(want[key]), key
        np.testing.assert_allclose(got[key], want[key], rtol=0, atol=1e-6, err_msg=str(key))
