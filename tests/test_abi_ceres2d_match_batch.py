"""CPU-side checks of cmx_ceres2d_match_grid_batch (CeresScanMatcher2D::Match for many robots in
one call, on resident probability grids and TSDFs alike): declared, listed, exported, mirrored with
the header's argument counts and the job struct's C layout, and every argument check made before
the device is touched -- with the index of the failing job in cmx_last_error and the outputs left
as they were.  The jobs here name stand-in grids; what needs a real grid (the results, a grid on
another device) is in tests/test_gpu_ceres2d_match_batch.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, PLAN = "cmx_ceres2d_match_grid_batch", "cmx_debug_ceres2d_batch_plan"
HEADER = os.path.join(ROOT, "include", "cartographer_mi355x.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "cartographer_mi355x_debug.h")


def _declaration(text, name):
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % name, stripped, re.S)
    assert m, f"{name} is not declared"
    return stripped, m


def test_header_declares_the_call_and_lists_it():
    text = open(HEADER).read()
    assert ENTRY in text.split("#ifndef")[0]                      # the entry-point list
    stripped, m = _declaration(text, ENTRY)
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 5
    # next to the 2D Ceres entries, before the 3D ones
    assert stripped.index("cmx_ceres2d_match_tsdf_grid(") < m.start() < stripped.index(
        "cmx_ceres3d_match(")
    assert "typedef struct cmx_ceres2d_job" in stripped
    _, m = _declaration(open(DEBUG_HEADER).read(), PLAN)
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 7


def test_library_exports_the_calls_and_the_mirrors_have_their_argument_counts():
    from cartographer_amd import _lib
    L = _lib.lib()
    assert ENTRY in _lib.EXPORTED_SYMBOLS and PLAN in _lib.DEBUG_SYMBOLS
    assert hasattr(L, ENTRY) and hasattr(L, PLAN)
    assert len(getattr(L, ENTRY).argtypes) == 5
    assert len(getattr(L, PLAN).argtypes) == 7


def _c_layout(tmp_path, header, struct, fields):
    src = tmp_path / f"{struct}.c"
    src.write_text(
        f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\n'
        f'int main(void) {{\n  printf("%zu", sizeof({struct}));\n' +
        "".join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in fields) +
        '  return 0;\n}\n')
    exe = str(tmp_path / struct)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe])
    return [int(w) for w in subprocess.run([exe], capture_output=True, text=True,
                                           check=True).stdout.split()]


def test_job_struct_has_the_layout_a_c99_compiler_gives_it(tmp_path):
    from cartographer_amd import _lib
    for mirror, header, struct in (
            (_lib.Ceres2DJob, "cartographer_mi355x.h", "cmx_ceres2d_job"),
            (_lib.DebugCeres2DJobPlan, "cartographer_mi355x_debug.h", "cmx_debug_ceres2d_job_plan"),
            (_lib.DebugCeres2DCallPlan, "cartographer_mi355x_debug.h",
             "cmx_debug_ceres2d_call_plan")):
        fields = [f[0] for f in mirror._fields_]
        words = _c_layout(tmp_path, header, struct, fields)
        assert words[0] == C.sizeof(mirror), struct
        assert words[1:] == [getattr(mirror, f).offset for f in fields], struct
    assert [f[0] for f in _lib.Ceres2DJob._fields_] == [
        "grid", "tsdf", "point_cloud_xyz", "cloud", "num_points", "reserved",
        "target_translation_xy", "initial_pose_estimate"]


def test_python_mirror_has_the_entry_points():
    from cartographer_amd import scan_matching as sm
    assert list(inspect.signature(sm.CeresScanMatcher2D.match_batch).parameters) == [
        "self", "target_translations", "initial_pose_estimates", "point_clouds", "grids"]
    assert list(inspect.signature(sm.ceres2d_batch_plan).parameters)[:2] == [
        "kinds", "point_clouds_or_counts"]


# ---- argument checks ------------------------------------------------------------------------
def _stand_in(device=0, num_points=0):
    """Zeroed memory with what a check reads of a handle: the device, the int every grid and
    cloud handle begins with, and -- of a cloud -- its number of points, the int behind it.  Its
    cell planes and points are null; no check looks at them, and no launch happens here."""
    buffer = C.create_string_buffer(4096)
    C.c_int32.from_buffer(buffer).value = device
    C.c_int32.from_buffer(buffer, 4).value = num_points
    return buffer


class _Call:
    """Five jobs (P, T, P, T, P) on stand-in grids; job 3 is a TSDF job without points, job 4
    names a stand-in resident cloud of 9 points."""
    SENTINEL = -7.0

    def __init__(self, num=5):
        from cartographer_amd import _lib
        self.lib = _lib
        self.num = num
        self.options = _lib.Ceres2DOptions(1.0, 10.0, 40.0, 0, 20)
        self.grids = [_stand_in() for _ in range(num)]
        self.cloud = _stand_in(num_points=9)
        self.points = [np.full((3 + k, 3), 0.5 + k, np.float32) for k in range(num)]
        self.jobs = (_lib.Ceres2DJob * num)()
        for k, job in enumerate(self.jobs):
            if k % 2:
                job.tsdf = C.addressof(self.grids[k])
            else:
                job.grid = C.addressof(self.grids[k])
            if k == 3:
                pass                                            # a TSDF job without points
            elif k == 4:
                job.cloud = C.addressof(self.cloud)
            else:
                job.point_cloud_xyz = self.points[k].ctypes.data
                job.num_points = self.points[k].shape[0]
            job.initial_pose_estimate = _lib.Pose2d(0.1 * k, -0.1 * k, 0.01 * k)
        self.poses = (_lib.Pose2d * num)()
        self.summaries = (_lib.CeresSummary * num)()
        for p, s in zip(self.poses, self.summaries):
            p.x = p.y = p.theta = s.initial_cost = s.final_cost = self.SENTINEL
            s.num_successful_steps = s.num_unsuccessful_steps = s.termination = int(self.SENTINEL)

    def __call__(self, **replace):
        a = dict(options=C.byref(self.options), jobs=self.jobs, num=self.num,
                 poses=C.cast(self.poses, C.c_void_p), summaries=C.cast(self.summaries, C.c_void_p))
        a.update(replace)
        return self.lib.lib().cmx_ceres2d_match_grid_batch(a["options"], a["jobs"], a["num"],
                                                           a["poses"], a["summaries"])

    def error(self):
        return self.lib.lib().cmx_last_error().decode()

    def untouched(self):
        return all(p.x == self.SENTINEL and p.y == self.SENTINEL and p.theta == self.SENTINEL
                   for p in self.poses) and all(
            s.initial_cost == self.SENTINEL and s.final_cost == self.SENTINEL and
            s.num_successful_steps == s.num_unsuccessful_steps == s.termination ==
            int(self.SENTINEL) for s in self.summaries)


def test_null_arrays_empty_lists_and_bad_options_are_invalid():
    call = _Call()
    for name in ("options", "jobs", "poses"):
        assert call(**{name: None}) == call.lib.INVALID_ARGUMENT, name
        assert call.untouched()
    assert call(num=0) == call.lib.INVALID_ARGUMENT
    assert "num_jobs" in call.error()
    assert call(num=-2) == call.lib.INVALID_ARGUMENT
    assert "num_jobs" in call.error()
    for field, value in (("occupied_space_weight", 0.0), ("translation_weight", -1.0),
                         ("rotation_weight", 0.0), ("max_num_iterations", 0)):
        call = _Call()
        setattr(call.options, field, value)
        assert call() == call.lib.INVALID_ARGUMENT, field
        assert call.untouched()


@pytest.mark.parametrize("index", [0, 2, 4])
def test_every_rule_names_the_job_first_middle_and_last(index):
    def broken(change, word):
        call = _Call()
        change(call, call.jobs[index])
        assert call() == call.lib.INVALID_ARGUMENT, word
        assert f"job {index}" in call.error() and word in call.error(), call.error()
        assert call.untouched()

    def no_kind(call, job):
        job.grid = job.tsdf = None

    def both_kinds(call, job):
        job.grid = job.tsdf = C.addressof(call.grids[index])

    def no_cloud(call, job):
        job.point_cloud_xyz = job.cloud = None
        job.num_points = 5

    def both_clouds(call, job):
        job.point_cloud_xyz = call.points[index].ctypes.data
        job.cloud = C.addressof(call.cloud)
        job.num_points = call.points[index].shape[0]

    def count(value):
        def change(call, job):
            job.point_cloud_xyz, job.cloud = call.points[index].ctypes.data, None
            job.num_points = value
        return change

    def resident_count(call, job):
        job.point_cloud_xyz, job.cloud = None, C.addressof(call.cloud)
        job.num_points = 8                                      # the cloud has 9

    def reserved(call, job):
        job.reserved = 1

    def other_device(call, job):
        C.c_int32.from_buffer(call.grids[index]).value = 1

    def cloud_on_other_device(call, job):
        other = _stand_in(device=1, num_points=9)
        call.keep = other
        job.point_cloud_xyz, job.cloud, job.num_points = None, C.addressof(other), 9

    broken(no_kind, "neither grid nor tsdf")
    broken(both_kinds, "both grid and tsdf")
    broken(no_cloud, "neither point_cloud_xyz nor cloud")
    broken(both_clouds, "both point_cloud_xyz and cloud")
    broken(count(0), "point count")                    # (jobs 0, 2, 4 are probability-grid jobs)
    broken(count(-1), "point count")
    broken(count(2**24 + 1), "point count")
    broken(resident_count, "count of its cloud")
    broken(reserved, "reserved")
    broken(cloud_on_other_device, "device")
    if index > 0:
        broken(other_device, "device")


@pytest.mark.parametrize("index", [1, 3])
def test_a_tsdf_job_takes_no_points_but_no_bad_count(index):
    for value in (-1, 2**24 + 1):
        call = _Call()
        call.jobs[index].point_cloud_xyz = call.points[index].ctypes.data
        call.jobs[index].num_points = value
        assert call() == call.lib.INVALID_ARGUMENT
        assert f"job {index}" in call.error() and "point count" in call.error(), call.error()
        assert call.untouched()


def test_one_pointer_with_two_counts_names_the_later_job():
    call = _Call()
    call.jobs[2].point_cloud_xyz = call.jobs[0].point_cloud_xyz     # 5 points against 3
    assert call() == call.lib.INVALID_ARGUMENT
    assert "job 2" in call.error() and "another point count" in call.error(), call.error()
    assert call.untouched()


def test_valid_arguments_reach_the_device():
    """Without a GPU the stand-ins pass every check and the call ends at the device.  With one,
    the same list on real grids (an empty 40 x 40 pair of them) runs: the stand-ins' null planes
    are nothing a kernel may read."""
    import torch
    call = _Call()
    if not torch.cuda.is_available():
        assert call() == call.lib.DEVICE_ERROR, call.error()
        assert "no CPU fallback" in call.error()
        assert call.untouched()
        return
    from cartographer_amd import grid_2d
    from cartographer_amd.scan_matching import PointCloudOnDevice
    grid = grid_2d.ProbabilityGridOnDevice(0.05, (1.0, 1.0), 40, 40)
    tsdf = grid_2d.TSDF2DOnDevice(0.05, (1.0, 1.0), 40, 40, 0.3, 10.0)
    cloud = PointCloudOnDevice(np.full((9, 3), 0.25, np.float32))
    for k, job in enumerate(call.jobs):
        if k % 2:
            job.tsdf = tsdf._h
        else:
            job.grid = grid._h
    call.jobs[4].cloud = cloud._h
    assert call() == call.lib.OK, call.error()
    assert not call.untouched()
    assert [s.termination for s in call.summaries][3] == 2       # the TSDF job without points
