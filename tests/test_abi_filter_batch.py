"""CPU-side checks of cmx_filter_batch (many voxel filters, and chains of them, in one call):
declared, exported, mirrored with the header's argument count and struct layouts, every argument
check made before the device is touched -- with the index of the failing job in cmx_last_error --
and the plan of a call (stage, launch, N and LDS bytes of every job, the staged clouds, the jobs
that run single) from the function the launch path itself asks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cmx_filter_batch"
PLAN = "cmx_debug_filter_batch_plan"
HEADER = os.path.join(ROOT, "include", "cartographer_mi355x.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "cartographer_mi355x_debug.h")
FIELDS = ["point_cloud_xyz", "num_points", "input_job", "mode", "length", "min_num_points",
          "max_range", "kept_indices", "filtered_xyz"]


def test_header_declares_the_call_and_lists_it():
    text = open(HEADER).read()
    assert NAME in text.split("#ifndef")[0]                       # the entry-point list
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % NAME, stripped, re.S)
    assert m, "not declared"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 4
    # in the point-preparation section, behind the single filters
    assert stripped.index("cmx_adaptive_voxel_filter_indices(") < m.start() < \
        stripped.index("cmx_compute_histogram(")
    assert re.search(r"enum\s*\{\s*CMX_FILTER_VOXEL\s*=\s*0\s*,\s*CMX_FILTER_ADAPTIVE\s*=\s*1\s*\}",
                     stripped)
    assert PLAN in open(DEBUG_HEADER).read()


def test_library_exports_the_call_and_the_mirror_has_its_argument_count():
    from cartographer_amd import _lib
    L = _lib.lib()
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert hasattr(L, NAME), f"{NAME} is not exported"
    assert len(getattr(L, NAME).argtypes) == 4
    assert PLAN in _lib.DEBUG_SYMBOLS
    assert len(getattr(L, PLAN).argtypes) == 4
    assert (_lib.FILTER_VOXEL, _lib.FILTER_ADAPTIVE) == (0, 1)


def _layout(tmp_path, header, struct, fields):
    """sizeof and member offsets of `struct` from a C99 program; compiling it -pedantic -Werror is
    also the check that the header is still plain C."""
    src = tmp_path / "size.c"
    src.write_text(
        f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\n'
        f'int main(void) {{\n  printf("%zu", sizeof({struct}));\n' +
        "".join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in fields) +
        '  return 0;\n}\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe])
    return [int(w) for w in subprocess.run([exe], capture_output=True, text=True,
                                           check=True).stdout.split()]


def test_job_struct_has_the_layout_a_c99_compiler_gives_it(tmp_path):
    from cartographer_amd import _lib
    assert [f[0] for f in _lib.FilterJob._fields_] == FIELDS
    words = _layout(tmp_path, "cartographer_mi355x.h", "cmx_filter_job", FIELDS)
    assert words[0] == C.sizeof(_lib.FilterJob)
    assert words[1:] == [getattr(_lib.FilterJob, f).offset for f in FIELDS]


@pytest.mark.parametrize("struct,mirror", [("cmx_debug_filter_job_plan", "DebugFilterJobPlan"),
                                           ("cmx_debug_filter_call_plan", "DebugFilterCallPlan")])
def test_plan_structs_have_the_layout_a_c99_compiler_gives_them(tmp_path, struct, mirror):
    from cartographer_amd import _lib
    mirror = getattr(_lib, mirror)
    fields = [f[0] for f in mirror._fields_]
    words = _layout(tmp_path, "cartographer_mi355x_debug.h", struct, fields)
    assert words[0] == C.sizeof(mirror)
    assert words[1:] == [getattr(mirror, f).offset for f in fields]


def test_python_mirror_has_the_entry_points():
    import inspect
    from cartographer_amd import filters
    parameters = inspect.signature(filters.filter_batch).parameters
    assert list(parameters) == ["jobs", "device"] and parameters["device"].default == 0
    assert list(inspect.signature(filters.filter_batch_plan).parameters) == ["jobs"]


def test_debug_switch_exists():
    from cartographer_amd import _lib
    try:
        _lib.debug_set(filter_batch_set_kb=64)
    finally:
        _lib.debug_reset()


# ---- argument checks ------------------------------------------------------------------------
class _Call:
    """Five valid jobs: three roots on host clouds (job 1 without outputs, jobs 3 and 4 chained on
    it), every output array with room for its root."""

    def __init__(self):
        from cartographer_amd import _lib
        self.lib = _lib
        self.num = 5
        self.clouds = [np.ones((7, 3), np.float32), np.ones((9, 3), np.float32),
                       np.ones((4, 3), np.float32)]
        self.indices = [np.zeros(16, np.int32) for _ in range(5)]
        self.points = [np.zeros((16, 3), np.float32) for _ in range(5)]
        self.items = (_lib.FilterJob * 5)()
        self.kept = (C.c_int32 * 5)()
        for k, item in enumerate(self.items):
            item.input_job = -1 if k < 3 else 1
            if k < 3:
                item.point_cloud_xyz = self.clouds[k].ctypes.data
                item.num_points = self.clouds[k].shape[0]
            item.mode = k % 2
            item.length, item.min_num_points, item.max_range = 0.5, 3.0, 50.0
            if k != 1:
                item.kept_indices = self.indices[k].ctypes.data
                item.filtered_xyz = self.points[k].ctypes.data

    def __call__(self, items="own", num=None, kept="own"):
        return self.lib.lib().cmx_filter_batch(
            self.items if items == "own" else items, self.num if num is None else num, 0,
            self.kept if kept == "own" else kept)

    def error(self):
        return self.lib.lib().cmx_last_error().decode()


def test_null_arguments_and_empty_lists_are_invalid():
    call = _Call()
    assert call(items=None) == call.lib.INVALID_ARGUMENT
    assert call(kept=None) == call.lib.INVALID_ARGUMENT
    assert call(num=0) == call.lib.INVALID_ARGUMENT
    assert "num_jobs" in call.error()
    assert call(num=-3) == call.lib.INVALID_ARGUMENT


def _broken(index, change):
    call = _Call()
    change(call.items[index], call)
    assert call() == call.lib.INVALID_ARGUMENT
    assert f"job {index}" in call.error(), call.error()


@pytest.mark.parametrize("index", [0, 2, 3, 4])
def test_rules_of_every_job_name_the_job(index):
    _broken(index, lambda item, call: setattr(item, "mode", 2))
    _broken(index, lambda item, call: setattr(item, "mode", -1))
    _broken(index, lambda item, call: setattr(item, "length", 0.0))
    _broken(index, lambda item, call: setattr(item, "length", -1.0))
    _broken(index, lambda item, call: setattr(item, "length", float("nan")))
    _broken(index, lambda item, call: setattr(item, "num_points", -1))
    _broken(index, lambda item, call: setattr(item, "num_points", 2**26 + 1))


@pytest.mark.parametrize("index", [0, 1, 2])
def test_rules_of_a_root_name_the_job(index):
    _broken(index, lambda item, call: setattr(item, "point_cloud_xyz", None))   # num_points > 0
    _broken(index, lambda item, call: setattr(item, "input_job", -2))


@pytest.mark.parametrize("index", [3, 4])
def test_rules_of_a_chained_job_name_the_job(index):
    _broken(index, lambda item, call: setattr(item, "point_cloud_xyz",
                                              call.clouds[0].ctypes.data))
    _broken(index, lambda item, call: setattr(item, "num_points", 7))
    _broken(index, lambda item, call: setattr(item, "input_job", index))        # itself
    _broken(index, lambda item, call: setattr(item, "input_job", 5))            # not earlier
    if index == 4:
        _broken(index, lambda item, call: setattr(item, "input_job", 3))        # not a root


def test_a_job_without_outputs_needs_a_job_chained_on_it():
    def strip(item, call):
        item.kept_indices = item.filtered_xyz = None
    for index in (0, 2, 3, 4):
        _broken(index, strip)
    # job 1 has none and is valid as long as a job chains on it
    call = _Call()
    call.items[3].input_job = call.items[4].input_job = 0
    assert call() == call.lib.INVALID_ARGUMENT
    assert "job 1" in call.error(), call.error()


def test_one_pointer_with_two_counts_is_named():
    call = _Call()
    call.items[2].point_cloud_xyz = call.clouds[0].ctypes.data                  # 4 points, not 7
    assert call() == call.lib.INVALID_ARGUMENT
    assert "job 2" in call.error(), call.error()


def test_the_largest_count_passes_the_checks():
    """2^26 points are valid (the plan makes the same checks and reads no cloud)."""
    call = _Call()
    call.items[0].num_points = 2**26
    plans = (call.lib.DebugFilterJobPlan * 5)()
    whole = call.lib.DebugFilterCallPlan()
    plan = call.lib.lib().cmx_debug_filter_batch_plan
    assert plan(call.items, 5, plans, C.byref(whole)) == call.lib.OK
    assert plans[0].single == 1 and plans[1].single == 0
    call.items[0].num_points = 2**26 + 1
    assert plan(call.items, 5, plans, C.byref(whole)) == call.lib.INVALID_ARGUMENT
    assert "job 0" in call.error()


def test_valid_arguments_reach_the_device():
    import torch
    call = _Call()
    status = call()
    if torch.cuda.is_available():
        assert status == call.lib.OK
    else:
        assert status == call.lib.DEVICE_ERROR, call.error()
    # empty clouds are valid too
    call = _Call()
    call.items[0].num_points = 0
    call.items[0].point_cloud_xyz = None
    assert call() == (call.lib.OK if torch.cuda.is_available() else call.lib.DEVICE_ERROR)


# ---- the plan -------------------------------------------------------------------------------
def _lds(N):
    """SmallFilterLdsBytes(N) + 5 N + 64: keys, indices and five int arrays of N, 64 wave totals
    and 64 bytes; behind them the active list (4 N) and the best result's flags (N)."""
    return N * (8 + 4 + 5 * 4) + 64 * 4 + 64 + 5 * N + 64


def _cloud(n):
    return np.zeros((n, 3), np.float32)


def test_plan_of_a_mixed_call():
    from cartographer_amd import filters
    shared = _cloud(1000)
    clouds = [_cloud(n) for n in (1, 64, 65, 2048, 2049, 4096, 5000)]
    jobs = [dict(cloud=c, mode="voxel", length=0.1) for c in clouds]              # 0 .. 6
    jobs += [dict(cloud=shared, mode="voxel", length=0.1, points=False, indices=False),   # 7
             dict(cloud=shared, mode="adaptive", length=0.5, min_num_points=200,
                  max_range=50.0),                                                # 8
             dict(cloud=_cloud(0), mode="voxel", length=0.1)]                     # 9
    chained = dict(mode="adaptive", length=0.5, min_num_points=100, max_range=50.0)
    jobs += [dict(chained, input_job=7), dict(chained, input_job=7),              # 10, 11
             dict(chained, input_job=5), dict(chained, input_job=6),              # 12, 13
             dict(chained, input_job=9), dict(chained, input_job=3)]              # 14, 15
    plans, call = filters.filter_batch_plan(jobs)

    want_N = [64, 64, 128, 2048, 4096, 4096, None, 1024, 1024, None,
              1024, 1024, 4096, None, None, 2048]
    for k, (plan, N) in enumerate(zip(plans, want_N)):
        assert plan["stage"] == (0 if k < 10 else 1), k
        if N is None:
            assert (plan["set"], plan["launch"], plan["N"], plan["lds_bytes"]) == (-1, -1, 0, 0), k
        else:
            assert plan["set"] == 0 and plan["N"] == N and plan["lds_bytes"] == _lds(N), k
            assert plan["launch"] == (0 if N <= 2048 else 1), k
    # the 5000-point root and its child run single, nothing else does
    assert [p["single"] for p in plans] == [int(k in (6, 13)) for k in range(16)]
    # one staged slot for equal pointers, none for chained jobs and the empty cloud
    slots = [p["cloud_slot"] for p in plans]
    assert slots[:9] == [0, 1, 2, 3, 4, 5, 6, 7, 7] and set(slots[9:]) == {-1}
    # both stages have both launch classes; the single jobs' cloud is not staged by the batch
    assert call["num_launches"] == 4 and call["num_sets"] == 1
    assert call["staged_bytes"] == 12 * (1 + 64 + 65 + 2048 + 2049 + 4096 + 1000)
    # N = 4096 fits the opt-in bound of the one-workgroup kernel, twice N = 2048 a compute unit
    assert _lds(4096) <= 160 * 1024 - 256 and 2 * _lds(2048) <= 160 * 1024


def test_plan_counts_only_the_launches_that_have_jobs():
    from cartographer_amd import filters
    jobs = [dict(cloud=_cloud(300), mode="voxel", length=0.1),
            dict(cloud=_cloud(0), mode="voxel", length=0.1),
            dict(input_job=1, mode="voxel", length=0.2)]
    plans, call = filters.filter_batch_plan(jobs)
    assert call == dict(staged_bytes=3600, num_launches=1, num_sets=1)
    assert [p["set"] for p in plans] == [0, -1, -1]
    # nothing but empty clouds: no set at all
    _, call = filters.filter_batch_plan(jobs[1:2])
    assert call == dict(staged_bytes=0, num_launches=0, num_sets=0)


def test_plan_cuts_a_call_into_sets_at_the_staging_bound_and_keeps_families_whole():
    from cartographer_amd import _lib, filters
    jobs = []
    for r in range(6):                              # 12000 bytes staged each, no result slots
        jobs.append(dict(cloud=_cloud(1000), mode="voxel", length=0.1, indices=False,
                         points=False))
    for r in range(6):                              # 4096 bytes of indices each
        jobs.append(dict(input_job=r, mode="adaptive", length=0.5, min_num_points=10,
                         max_range=50.0, points=False))
    try:
        _lib.debug_set(filter_batch_set_kb=30)        # two clouds per set
        plans, call = filters.filter_batch_plan(jobs)
    finally:
        _lib.debug_reset()
    assert [p["set"] for p in plans] == [0, 0, 1, 1, 2, 2] * 2
    assert call == dict(staged_bytes=72000, num_launches=6, num_sets=3)
    plans, call = filters.filter_batch_plan(jobs)
    assert {p["set"] for p in plans} == {0} and call["num_launches"] == 2


def test_plan_reports_the_errors_of_the_call():
    from cartographer_amd import _lib, filters
    with pytest.raises(_lib.CmxError) as e:
        filters.filter_batch_plan([dict(cloud=_cloud(5), mode="voxel", length=0.1),
                                   dict(cloud=_cloud(5), mode="voxel", length=0.0)])
    assert e.value.status == _lib.INVALID_ARGUMENT and "job 1" in str(e.value)


def test_host_planning_holds_its_invariants_under_sanitizers(tmp_path):
    """filters_batch_plan.h as a stand-alone program under the address and undefined-behaviour
    sanitizers: random forests of jobs, every descriptor slot given out once, launches that tile
    a set's table, families in one set, the checks' verdicts on broken lists."""
    exe = tmp_path / "filter_batch_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cartographer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "filter_batch_plan_check.cc"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "calls 2000" in out.stdout and "failures 0" in out.stdout
