"""The reference's LocalTrajectoryBuilder2D, unmodified, in TSDF mode (grid_type = "TSDF"):
examples/dropin/local_trajectory_builder_2d_main.cc built with -DDROPIN_TSDF three ways --
the reference's own matchers and TSDFRangeDataInserter2D (the golden drive), the adapters over the
product library (TSDF Ceres refinement through cmx_ceres2d_match_tsdf), and the resident build
whose submaps are cmx_tsdf2d handles (insert, crop, cmx_rt2d_match_tsdf_grid,
cmx_ceres2d_match_tsdf_grid; only the clouds cross PCIe).  Same bar as tests/test_dropin.py's
probability-grid drive."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "examples", "dropin")
DROPIN_BUILD = os.path.join(ROOT, "oracle", "_ref", "dropin")
REFERENCE = "/root/reference"
TSDF_REFERENCE = os.path.join(DROPIN_BUILD, "local_trajectory_builder_2d_tsdf_reference")
TSDF_MI355X = os.path.join(DROPIN_BUILD, "local_trajectory_builder_2d_tsdf_mi355x")
TSDF_RESIDENT = os.path.join(DROPIN_BUILD, "local_trajectory_builder_2d_tsdf_resident_mi355x")
TSDF_GOLDEN = os.path.join(ROOT, "tests", "golden", "local_trajectory_builder_2d_tsdf_reference.txt")


def _drive(text):
    """(scan index, [x, y, yaw], points matched, submaps inserted into) of every result line,
    the submap digests (scans, finished, cells x, cells y, known, tsd sum), the worst distance
    from the simulated truth."""
    poses, submaps, worst = [], [], None
    for line in text.splitlines():
        w = line.split()
        if line.startswith("scan") and "pose" in line:
            poses.append((int(w[1]), [float(v) for v in w[5:8]], int(w[13]), int(w[15])))
        elif line.startswith("submap"):
            submaps.append((int(w[2]), int(w[4]), int(w[6]), int(w[8]), int(w[10]), float(w[12])))
        elif line.startswith("results"):
            worst = float(w[5])
    return poses, submaps, worst


def test_golden_tsdf_drive_follows_the_truth():
    """The committed reference drive: 79 results, a second submap filled, within 4 cm of the
    simulated truth."""
    poses, submaps, worst = _drive(open(TSDF_GOLDEN).read())
    assert len(poses) == 79 and worst < 0.04
    assert sum(1 for p in poses if p[3] == 2) > 20
    assert len(submaps) == 2


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree to compile")
def test_tsdf_reference_drive_reproduces_its_golden():
    """The reference build (its own real-time and Ceres matchers, TSDF2D and
    TSDFRangeDataInserter2D) prints the committed golden byte for byte."""
    subprocess.run(["make", "-C", DROPIN, f"OUT={DROPIN_BUILD}", TSDF_REFERENCE], check=True,
                   capture_output=True)
    out = subprocess.run([TSDF_REFERENCE], check=True, capture_output=True,
                         timeout=120).stdout
    assert out == open(TSDF_GOLDEN, "rb").read()


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree to compile")
def test_tsdf_device_builds_link_the_device_calls():
    """The adapters' build refines through cmx_ceres2d_match_tsdf; the resident build inserts and
    matches through the cmx_tsdf2d handle and does not link the reference's TSDF inserter."""
    subprocess.run(["make", "-C", DROPIN, f"OUT={DROPIN_BUILD}", TSDF_MI355X, TSDF_RESIDENT],
                   check=True, capture_output=True)
    symbols = subprocess.run(["nm", "-C", TSDF_MI355X], check=True, capture_output=True,
                             text=True).stdout
    for name in ("cmx_rt2d_match_tsdf", "cmx_ceres2d_match_tsdf"):
        assert name in symbols
    assert "TSDFRangeDataInserter2D::Insert" in symbols
    symbols = subprocess.run(["nm", "-C", TSDF_RESIDENT], check=True, capture_output=True,
                             text=True).stdout
    for name in ("cmx_tsdf2d_create", "cmx_tsdf2d_insert", "cmx_tsdf2d_crop",
                 "cmx_rt2d_match_tsdf_grid", "cmx_ceres2d_match_tsdf_grid"):
        assert name in symbols
    assert "TSDFRangeDataInserter2D::Insert" not in symbols
    assert "LocalTrajectoryBuilder2D::AddAccumulatedRangeData" in symbols


@pytest.mark.gpu
@pytest.mark.parametrize("binary", ["adapters", "resident"])
def test_tsdf_drive_on_the_gpu_follows_the_references_drive(binary):
    """The same 80 scans in TSDF mode with the device under the unmodified builder: the first ten
    results agree with the golden to 1e-6, all of them to 5 mm, the same scans go into the same
    number of submaps, and the drive stays as close to the truth as the reference's."""
    path = TSDF_MI355X if binary == "adapters" else TSDF_RESIDENT
    assert os.path.exists(path), "oracle/_ref/dropin is prebuilt by __graft_entry__.build()"
    run = subprocess.run([path], check=True, capture_output=True, text=True, timeout=300)
    got, got_submaps, got_worst = _drive(run.stdout)
    want, want_submaps, want_worst = _drive(open(TSDF_GOLDEN).read())
    assert len(got) == len(want) == 79
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[3] == w[3]
        np.testing.assert_allclose(g[1], w[1], rtol=0, atol=1e-6 if k < 10 else 5e-3)
        assert abs(g[2] - w[2]) <= 3                   # points the adaptive filter kept
    assert abs(got_worst - want_worst) < 5e-3
    assert len(got_submaps) == len(want_submaps) == 2
    for g, w in zip(got_submaps, want_submaps):
        assert g[:4] == w[:4]                          # scans, finished, cells
        assert abs(g[4] - w[4]) <= 0.01 * w[4] and abs(g[5] - w[5]) <= 0.01 * abs(w[5])
    print(run.stderr.strip())                          # ms per AddRangeData
