"""CPU-side checks of cmx_compute_histogram_batch (the rotational histograms of many clouds in
one call): declared, exported, mirrored with the header's argument count and struct layouts, every
argument check made before the device is touched -- with the index of the failing job in
cmx_last_error -- and the plan of a call (route, set, launch, slot, N and LDS bytes of every job,
the staged clouds) from the function the launch path itself asks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cmx_compute_histogram_batch"
PLAN = "cmx_debug_histogram_batch_plan"
HEADER = os.path.join(ROOT, "include", "cartographer_mi355x.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "cartographer_mi355x_debug.h")
FIELDS = ["point_cloud_xyz", "num_points", "histogram_size", "histogram"]
NONE, BATCHED, SINGLE = 0, 1, 2


def test_header_declares_the_call_and_lists_it():
    text = open(HEADER).read()
    assert NAME in text.split("#ifndef")[0]                       # the entry-point list
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % NAME, stripped, re.S)
    assert m, "not declared"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 3
    # in the point-preparation section, behind the single histogram
    assert stripped.index("cmx_compute_histogram(") < m.start() < stripped.index("cmx_comm_init(")
    debug = open(DEBUG_HEADER).read()
    assert PLAN in debug
    assert re.search(r"enum\s*\{\s*CMX_HISTOGRAM_NONE\s*=\s*0\s*,\s*CMX_HISTOGRAM_BATCHED\s*=\s*1\s*,"
                     r"\s*CMX_HISTOGRAM_SINGLE\s*=\s*2\s*\}", debug)


def test_library_exports_the_call_and_the_mirror_has_its_argument_count():
    from cartographer_amd import _lib
    L = _lib.lib()
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert hasattr(L, NAME), f"{NAME} is not exported"
    assert len(getattr(L, NAME).argtypes) == 3
    assert PLAN in _lib.DEBUG_SYMBOLS
    assert len(getattr(L, PLAN).argtypes) == 4
    assert (_lib.HISTOGRAM_NONE, _lib.HISTOGRAM_BATCHED, _lib.HISTOGRAM_SINGLE) == (0, 1, 2)


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
    assert [f[0] for f in _lib.HistogramJob._fields_] == FIELDS
    words = _layout(tmp_path, "cartographer_mi355x.h", "cmx_histogram_job", FIELDS)
    assert words[0] == C.sizeof(_lib.HistogramJob)
    assert words[1:] == [getattr(_lib.HistogramJob, f).offset for f in FIELDS]


@pytest.mark.parametrize("struct,mirror",
                         [("cmx_debug_histogram_job_plan", "DebugHistogramJobPlan"),
                          ("cmx_debug_histogram_call_plan", "DebugHistogramCallPlan")])
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
    parameters = inspect.signature(filters.compute_histogram_batch).parameters
    assert list(parameters) == ["clouds", "histogram_size", "device"]
    assert parameters["device"].default == 0
    assert list(inspect.signature(filters.histogram_batch_plan).parameters) == \
        ["clouds", "histogram_size"]


def test_debug_switch_exists():
    from cartographer_amd import _lib
    try:
        _lib.debug_set(histogram_batch_set_kb=64)
    finally:
        _lib.debug_reset()


# ---- argument checks ------------------------------------------------------------------------
SENTINEL = -7.0


class _Call:
    """Five valid jobs: jobs 1 and 3 on one cloud with two sizes, job 4 without points."""

    def __init__(self):
        from cartographer_amd import _lib
        self.lib = _lib
        self.num = 5
        self.clouds = [np.ones((7, 3), np.float32), np.ones((9, 3), np.float32),
                       np.ones((4, 3), np.float32)]
        self.outputs = [np.full(128, SENTINEL, np.float32) for _ in range(5)]
        self.items = (_lib.HistogramJob * 5)()
        for k, (cloud, size) in enumerate([(0, 120), (1, 120), (2, 16), (1, 7), (None, 33)]):
            item = self.items[k]
            if cloud is not None:
                item.point_cloud_xyz = self.clouds[cloud].ctypes.data
                item.num_points = self.clouds[cloud].shape[0]
            item.histogram_size = size
            item.histogram = self.outputs[k].ctypes.data

    def __call__(self, items="own", num=None):
        return self.lib.lib().cmx_compute_histogram_batch(
            self.items if items == "own" else items, self.num if num is None else num, 0)

    def error(self):
        return self.lib.lib().cmx_last_error().decode()

    def untouched(self):
        return all((out == SENTINEL).all() for out in self.outputs)


def test_null_jobs_and_empty_lists_are_invalid():
    call = _Call()
    assert call(items=None) == call.lib.INVALID_ARGUMENT
    assert "jobs" in call.error()
    assert call(num=0) == call.lib.INVALID_ARGUMENT
    assert "num_jobs" in call.error()
    assert call(num=-3) == call.lib.INVALID_ARGUMENT
    assert call.untouched()


def _broken(index, change):
    call = _Call()
    change(call.items[index], call)
    assert call() == call.lib.INVALID_ARGUMENT
    assert f"job {index}" in call.error(), call.error()
    assert call.untouched()


@pytest.mark.parametrize("index", [0, 1, 2, 3, 4])
def test_rules_of_every_job_name_the_job(index):
    _broken(index, lambda item, call: setattr(item, "num_points", -1))
    _broken(index, lambda item, call: setattr(item, "num_points", 2**24 + 1))
    _broken(index, lambda item, call: setattr(item, "histogram_size", 0))
    _broken(index, lambda item, call: setattr(item, "histogram_size", -5))
    _broken(index, lambda item, call: setattr(item, "histogram_size", 8193))
    _broken(index, lambda item, call: setattr(item, "histogram", None))


@pytest.mark.parametrize("index", [0, 1, 2, 3])
def test_a_null_cloud_with_points_names_the_job(index):
    _broken(index, lambda item, call: setattr(item, "point_cloud_xyz", None))


def test_one_pointer_with_two_counts_is_named():
    call = _Call()
    call.items[3].num_points = 8                                        # job 1 says 9
    assert call() == call.lib.INVALID_ARGUMENT
    assert "job 3" in call.error(), call.error()
    assert call.untouched()


def test_the_limits_themselves_pass_the_checks():
    """2^24 points and 8192 bins are valid (the plan makes the same checks; it reads the clouds of
    up to 4096 points only)."""
    call = _Call()
    call.items[0].num_points = 2**24
    call.items[2].histogram_size = 8192
    plans = (call.lib.DebugHistogramJobPlan * 5)()
    whole = call.lib.DebugHistogramCallPlan()
    plan = call.lib.lib().cmx_debug_histogram_batch_plan
    assert plan(call.items, 5, plans, C.byref(whole)) == call.lib.OK
    assert [p.route for p in plans] == [SINGLE, BATCHED, BATCHED, BATCHED, NONE]
    assert plan(call.items, 5, None, C.byref(whole)) == call.lib.INVALID_ARGUMENT
    assert plan(call.items, 5, plans, None) == call.lib.INVALID_ARGUMENT
    call.items[0].num_points = 2**24 + 1
    assert plan(call.items, 5, plans, C.byref(whole)) == call.lib.INVALID_ARGUMENT
    assert "job 0" in call.error()


def test_valid_arguments_reach_the_device():
    import torch
    call = _Call()
    status = call()
    if torch.cuda.is_available():
        assert status == call.lib.OK
        assert not call.outputs[4][:33].any() and (call.outputs[4][33:] == SENTINEL).all()
    else:
        assert status == call.lib.DEVICE_ERROR, call.error()
    # nothing but empty clouds is valid too
    call = _Call()
    for item in call.items:
        item.num_points, item.point_cloud_xyz = 0, None
    assert call() == (call.lib.OK if torch.cuda.is_available() else call.lib.DEVICE_ERROR)


# ---- the plan -------------------------------------------------------------------------------
def _lds(N):
    """HistogramLdsBytes(N): 64-bit keys, four coordinate rows and three int arrays of N, 64 wave
    totals and 64 bytes."""
    return N * (8 + 4 * 4 + 3 * 4) + 64 * 4 + 64


def _per_unit(N):
    """Workgroups a compute unit holds: 160 KB of LDS, and the kernel's registers admit one
    workgroup of 1024 threads."""
    return min(1, (160 * 1024) // _lds(N))


def _classes():
    """The launch class of every carve: one more behind every N at which _per_unit changes."""
    classes, cls = {64: 0}, 0
    for N in (128, 256, 512, 1024, 2048, 4096):
        cls += _per_unit(N) != _per_unit(N // 2)
        classes[N] = cls
    return classes


def _cloud(n):
    return np.zeros((n, 3), np.float32)


def test_plan_of_a_mixed_call():
    from cartographer_amd import filters
    shared = _cloud(1000)
    poisoned = _cloud(300)
    poisoned[299, 1] = np.nan
    infinite = _cloud(4096)
    infinite[0, 0] = -np.inf
    clouds = [_cloud(n) for n in (0, 1, 64, 65, 2048, 2049, 4096, 4097)]      # 0 .. 7
    clouds += [shared, poisoned, shared, infinite, poisoned]                  # 8 .. 12
    sizes = [120] * 8 + [120, 120, 7, 8192, 16]
    plans, call = filters.histogram_batch_plan(clouds, sizes)

    want_route = [NONE] + [BATCHED] * 6 + [SINGLE, BATCHED, SINGLE, BATCHED, SINGLE, SINGLE]
    want_N = [0, 64, 64, 128, 2048, 4096, 4096, 0, 1024, 0, 1024, 0, 0]
    classes = _classes()
    assert [p["route"] for p in plans] == want_route
    assert [p["N"] for p in plans] == want_N
    for k, plan in enumerate(plans):
        if plan["route"] == BATCHED:
            assert plan["set"] == 0 and plan["lds_bytes"] == _lds(plan["N"]), k
            assert plan["launch"] == sorted(set(classes[N] for N in want_N if N)).index(
                classes[plan["N"]]), k
        else:
            assert (plan["set"], plan["launch"], plan["slot"], plan["lds_bytes"]) == (-1, -1, -1, 0), k
    # every batched job one slot; the slots of a launch follow each other in list order
    batched = [k for k, p in enumerate(plans) if p["route"] == BATCHED]
    assert sorted(plans[k]["slot"] for k in batched) == list(range(len(batched)))
    by_slot = sorted(batched, key=lambda k: plans[k]["slot"])
    assert by_slot == sorted(batched, key=lambda k: (plans[k]["launch"], k))
    # one staged slot for equal pointers, none for the empty cloud
    assert [p["cloud_slot"] for p in plans] == [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 7, 9, 8]
    # the single jobs' clouds are not staged by the batch, a shared cloud once
    assert call["staged_bytes"] == 12 * (1 + 64 + 65 + 2048 + 2049 + 4096 + 1000)
    assert call["num_sets"] == 1
    assert call["num_launches"] == len(set(classes[N] for N in want_N if N))
    # the largest carve fits the opt-in bound of the kernel and a compute unit
    assert _lds(4096) <= 160 * 1024 - 256
    assert all(_per_unit(N) >= 1 for N in classes)


def test_plan_without_batched_jobs_has_no_set():
    from cartographer_amd import filters
    plans, call = filters.histogram_batch_plan([_cloud(0), _cloud(5000)], [120, 7])
    assert [p["route"] for p in plans] == [NONE, SINGLE]
    assert call == dict(staged_bytes=0, num_launches=0, num_sets=0)


def test_plan_cuts_a_call_into_sets_at_the_bounds():
    from cartographer_amd import _lib, filters
    clouds = [_cloud(1000) for _ in range(6)]                 # 12000 bytes staged each
    try:
        _lib.debug_set(histogram_batch_set_kb=30)             # two clouds per set
        plans, call = filters.histogram_batch_plan(clouds, 120)
        assert [p["set"] for p in plans] == [0, 0, 1, 1, 2, 2]
        assert [p["slot"] for p in plans] == [0, 1] * 3
        assert call == dict(staged_bytes=72000, num_launches=3, num_sets=3)
        # ... and at the result block: 8192 bins are 32 KB of it
        _lib.debug_set(histogram_batch_set_kb=70)
        plans, call = filters.histogram_batch_plan(clouds, 8192)
        assert [p["set"] for p in plans] == [0, 0, 1, 1, 2, 2]
    finally:
        _lib.debug_reset()
    plans, call = filters.histogram_batch_plan(clouds, 120)
    assert {p["set"] for p in plans} == {0} and call["num_launches"] == 1


def test_plan_reports_the_errors_of_the_call():
    from cartographer_amd import _lib, filters
    with pytest.raises(_lib.CmxError) as e:
        filters.histogram_batch_plan([_cloud(5), _cloud(5)], [120, 0])
    assert e.value.status == _lib.INVALID_ARGUMENT and "job 1" in str(e.value)
