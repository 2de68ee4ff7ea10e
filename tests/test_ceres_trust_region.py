"""ceres_trust_region.h (the trust-region Levenberg-Marquardt loop and the Cholesky solve that
Ceres2DKernel and Ceres3DKernel share) as a stand-alone program under the address and
undefined-behaviour sanitizers: run over oracle::CeresResiduals2D on a small grid built in code, it
must return the pose, both costs, both step counts and the termination of
oracle::CeresScanMatcher2DMatch with == (the same statements over the same sums, one compiler,
-ffp-contract=off) for converging solves, rejected steps, monotonic and not, iteration caps 1 - 3
and a zero gradient; a failing evaluator follows the kernels' rules; and every case gives the same
bits through the 3D kernel's instantiation (array bound 6, three unknowns).  The GPU tests of the
entry points (test_gpu_ceres_edges.py, test_gpu_ceres_tsdf.py) pin the kernels around it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_minimizer_equals_the_oracle_under_sanitizers(tmp_path):
    exe = tmp_path / "ceres_trust_region_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cartographer_amd", "csrc"),
                    "-I", os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tests", "native", "ceres_trust_region_check.cc"),
                    os.path.join(ROOT, "oracle", "oracle_ceres_2d.cc"),
                    os.path.join(ROOT, "oracle", "oracle_2d.cc"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "failures 0" in out.stdout
    assert int(re.search(r"cases (\d+)", out.stdout).group(1)) == 10
