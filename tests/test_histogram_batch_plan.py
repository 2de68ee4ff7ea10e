"""histogram_batch_plan.h (the host's plan of cmx_compute_histogram_batch: routes, LDS carves,
launch classes, sets and descriptor slots) as a stand-alone program under the address and
undefined-behaviour sanitizers: every batched job of random job lists has exactly one slot in
exactly one set, the slots of a launch are contiguous, a launch's N is the largest of its jobs and
within its class, no set passes its bounds unless a single job does so alone, equal pointers share
a cloud slot, and the LDS of the largest carve stays at or below a compute unit's 160 KB.  The GPU
tests of the call (tests/test_gpu_histogram_batch.py) pin the kernel against the single call."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_histogram_batch_plan_holds_its_invariants_under_sanitizers(tmp_path):
    exe = tmp_path / "histogram_batch_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cartographer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "histogram_batch_plan_check.cc"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "failures 0" in out.stdout
    assert int(re.search(r"calls (\d+)", out.stdout).group(1)) == 2000
    assert int(re.search(r"sets (\d+)", out.stdout).group(1)) > 2000
