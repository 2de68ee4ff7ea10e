"""ceres_2d_batch_plan.h (the host's plan of cmx_ceres2d_match_grid_batch: the job checks that
need no grid, and the layout of the call's one upload block) -- through cmx_debug_ceres2d_batch_plan,
which asks the function the launch path asks and needs no device, and as a stand-alone program
under the address and undefined-behaviour sanitizers (tests/native/ceres2d_batch_plan_check.cc).
The GPU tests of the call (tests/test_gpu_ceres2d_match_batch.py) pin the kernel against the
single calls."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, T = 0, 1


def _plan(kinds, clouds, resident=None):
    from cartographer_amd.scan_matching import ceres2d_batch_plan
    return ceres2d_batch_plan(kinds, clouds, resident)


def _align(n):
    return (n + 255) & ~255


def test_jobs_naming_one_host_pointer_share_one_slot():
    a, b = np.zeros((200, 3), np.float32), np.zeros((63, 3), np.float32)
    jobs, call = _plan([T, P, T, P, P], [a, b, a, b, a])
    assert [j["cloud_slot"] for j in jobs] == [0, 1, 0, 1, 0]
    assert jobs[0]["cloud_offset"] == jobs[2]["cloud_offset"] == jobs[4]["cloud_offset"]
    assert jobs[1]["cloud_offset"] == jobs[3]["cloud_offset"] != jobs[0]["cloud_offset"]
    assert call["num_clouds"] == 2
    # first-seen order, one behind the other from 256-byte boundaries behind the problem array
    assert jobs[0]["cloud_offset"] == call["problem_bytes"]
    assert jobs[1]["cloud_offset"] == call["problem_bytes"] + _align(12 * 200)
    # an equal array that is another object is another cloud
    jobs, call = _plan([P, P], [a, a.copy()])
    assert [j["cloud_slot"] for j in jobs] == [0, 1] and call["num_clouds"] == 2


def test_resident_and_empty_clouds_take_no_slot():
    a = np.zeros((21, 3), np.float32)
    # job 1: resident, 300 points; job 2: a TSDF job without points; job 4: resident
    jobs, call = _plan([P, P, T, T, T], [a, 300, 0, a, 64], resident=[0, 1, 0, 0, 1])
    assert [j["cloud_slot"] for j in jobs] == [0, -1, -1, 0, -1]
    assert [j["cloud_offset"] for j in jobs[1:3]] == [0, 0] and jobs[4]["cloud_offset"] == 0
    assert call["num_clouds"] == 1
    assert call["total_bytes"] == call["problem_bytes"] + _align(12 * 21)
    # nothing but resident and empty clouds: the block is the problem array
    jobs, call = _plan([P, T, T], [5, 0, 7], resident=[1, 0, 1])
    assert call["num_clouds"] == 0 and call["total_bytes"] == call["problem_bytes"]


def test_total_is_the_aligned_problem_array_plus_the_distinct_clouds():
    rng = np.random.default_rng(3)
    sizes = [1, 21, 22, 63, 64, 200, 255, 256, 257, 1000]
    clouds = [np.zeros((n, 3), np.float32) for n in sizes]
    previous = 0
    for num in (1, 2, 7, 40, 300):
        picks = rng.integers(0, len(clouds), num)
        kinds = rng.integers(0, 2, num)
        jobs, call = _plan(kinds, [clouds[k] for k in picks])
        distinct = list(dict.fromkeys(int(k) for k in picks))
        assert call["num_clouds"] == len(distinct)
        assert call["total_bytes"] == call["problem_bytes"] + sum(
            _align(12 * sizes[k]) for k in distinct)
        offsets = [call["problem_bytes"]]
        for k in distinct:
            offsets.append(offsets[-1] + _align(12 * sizes[k]))
        assert [j["cloud_offset"] for j in jobs] == [offsets[distinct.index(int(k))] for k in picks]
        # the problem array: to a 256-byte boundary, decided by the number of jobs alone
        assert call["problem_bytes"] % 256 == 0 and call["problem_bytes"] >= max(previous, 8 * num)
        previous = call["problem_bytes"]
        assert _plan([P] * num, [5] * num, [1] * num)[1]["problem_bytes"] == previous


def test_launch_count_does_not_grow_with_the_jobs():
    a = np.zeros((50, 3), np.float32)
    counts = []
    for num in (1, 7, 300):
        kinds = [(T, P)[k % 2] for k in range(num)]
        _, call = _plan(kinds, [a if k % 3 == 0 else 10 + k for k in range(num)])
        counts.append(call["num_launches"])
    assert counts[0] == counts[1] == counts[2]
    assert 1 <= counts[0] <= 2
    for kinds in ([P] * 5, [T] * 5):                       # one kind only: the same launches
        assert _plan(kinds, [a] * 5)[1]["num_launches"] == counts[0]


def test_kinds_come_back_in_list_order():
    kinds = [T, P, T, P, P, T, P]
    jobs, _ = _plan(kinds, [1, 63, 64, 255, 256, 257, 200])
    assert [j["kind"] for j in jobs] == kinds
    assert [j["cloud_slot"] for j in jobs] == list(range(7))       # ints: a cloud of its own each


def test_one_pointer_with_two_counts_names_the_later_job():
    from cartographer_amd import _lib
    a = np.zeros((200, 3), np.float32)
    b = np.zeros((10, 3), np.float32)
    with pytest.raises(_lib.CmxError) as e:
        _plan([P, T, P, P], [a, b, b, (a, 199)])
    assert e.value.status == _lib.INVALID_ARGUMENT
    assert "job 3" in str(e.value) and "job 0" not in str(e.value)
    with pytest.raises(_lib.CmxError) as e:
        _plan([P, T, P, P], [a, (a, 100), b, a])
    assert "job 1" in str(e.value)


@pytest.mark.parametrize("index", [0, 2, 4])
def test_the_entrys_errors_that_the_plan_can_see(index):
    from cartographer_amd import _lib
    a = np.zeros((30, 3), np.float32)

    def refused(kinds, clouds, resident, word):
        with pytest.raises(_lib.CmxError) as e:
            _plan(kinds, clouds, resident)
        assert e.value.status == _lib.INVALID_ARGUMENT
        assert f"job {index}" in str(e.value) and word in str(e.value), str(e.value)

    kinds, clouds, resident = [P, T, P, T, P], [a, 5, a, 0, 9], [0, 0, 0, 0, 0]

    def with_(at, kind=None, cloud=None, flag=None):
        k, c, r = list(kinds), list(clouds), list(resident)
        if kind is not None:
            k[at] = kind
        if cloud is not None:
            c[at] = cloud
        if flag is not None:
            r[at] = flag
        return k, c, r

    refused(*with_(index, kind=2), "kind")
    refused(*with_(index, kind=P, cloud=(a, 0)), "point count")        # no points on a probability grid
    refused(*with_(index, cloud=(a, 2**24 + 1)), "point count")
    refused(*with_(index, cloud=(a, -1)), "point count")
    refused(*with_(index, cloud=(a, 30), flag=1), "both")             # a host cloud and a resident one
    refused(*with_(index, cloud=(np.zeros((0, 3), np.float32), 5)), "neither")
    # a TSDF job takes 0 points and the full 2^24
    _plan(*with_(index, kind=T, cloud=0))
    _plan(*with_(index, kind=T, cloud=(np.zeros((1, 3), np.float32), 2**24)))


def test_ceres2d_batch_plan_holds_its_invariants_under_sanitizers(tmp_path):
    exe = tmp_path / "ceres2d_batch_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cartographer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "ceres2d_batch_plan_check.cc"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "failures 0" in out.stdout
    assert int(re.search(r"calls (\d+)", out.stdout).group(1)) == 2000
    assert int(re.search(r"slots (\d+)", out.stdout).group(1)) > 2000
