"""cmx_batch.h (what the batched calls share: block-to-entry bisection, set cutting, staging of
host arrays by pointer, upload-block layout) on the host, as a stand-alone program under the
address and undefined-behaviour sanitizers.  The header's device part is the same text: the GPU
tests of the four batched calls pin it against the single calls."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_toolkit_holds_its_invariants_under_sanitizers(tmp_path):
    exe = tmp_path / "batch_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cartographer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "batch_plan_check.cc"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "tables 5454" in out.stdout and "failures 0" in out.stdout
