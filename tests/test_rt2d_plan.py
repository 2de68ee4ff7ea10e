"""rt_2d_plan.h (the host's plan of a real-time 2D tile-matcher call: tile geometry, every LDS size
of its kernels, work items, launch grid, scratch offsets and the layout of the upload block) as a
stand-alone program under the address and undefined-behaviour sanitizers.  Every output field of a
fixed case list -- windows, clouds, grids, two window classes, several tiles, the re-plan, batch
sizes, shares and the debug switches, the ineligible outcomes included -- must equal the record in
tests/golden/rt2d_plan_parent.json, which was written by the statements of Rt2DTileCall::Plan() and
Enqueue() as they stood before the header existed; every eligible case must also keep its LDS
within the launches' budgets, its pitches conflict-free and its staging regions disjoint."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rt2d_plan_parent.json")


def test_rt2d_plan_equals_the_parent_record_under_sanitizers(tmp_path):
    exe = tmp_path / "rt2d_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cartographer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "rt2d_plan_check.cc"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), GOLDEN], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "failures 0" in out.stdout
    with open(GOLDEN) as f:
        recorded = json.load(f)["cases"]
    names = [c["name"] for c in recorded]
    assert len(recorded) >= 60 and len(set(names)) == len(names)
    assert int(re.search(r"cases (\d+)", out.stdout).group(1)) == len(recorded)
    # (the re-plan and the several-tile shapes are recorded as plans, not as refusals)
    assert all(c["eligible"] == 1 for c in recorded if c["name"] in ("replan", "long_range", "two_classes"))
    assert int(re.search(r"fields compared (\d+)", out.stdout).group(1)) > 5000


def test_rt2d_plan_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "alone.cc"
    src.write_text('#include "rt_2d_plan.h"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "cartographer_amd", "csrc"), str(src), "-o",
                    str(tmp_path / "alone")], check=True)
