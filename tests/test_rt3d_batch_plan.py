"""rt_3d_batch_plan.h (the host's plan of cmx_rt3d_match_grid_batch: search windows, routes, launch
sets and the blocks of every match) as a stand-alone program under the address and
undefined-behaviour sanitizers: every block of random match lists is owned by the right match,
one-block matches, a set cut at each of its three bounds, a match that exceeds a bound alone,
strictly increasing first blocks.  The device asks the same bisection (cmx_batch.h); the GPU tests
of the call pin it against the single calls."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rt3d_batch_plan_holds_its_invariants_under_sanitizers(tmp_path):
    exe = tmp_path / "rt3d_batch_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cartographer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "rt3d_batch_plan_check.cc"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "failures 0" in out.stdout
    asked = int(re.search(r"blocks asked (\d+)", out.stdout).group(1))
    assert asked > 100000
