"""CPU-side checks of cmx_rt3d_match_grid_batch and cmx_ceres3d_match_grids_batch (the two halves
of LocalTrajectoryBuilder3D::ScanMatch for many trajectories in one call each): declared, exported,
mirrored with the header's argument counts, every argument check made before the device is touched
-- with the index of the failing match in cmx_last_error -- and the plan of a real-time call (the
window, route, launch set and blocks of every match) from the functions the launch path asks.

The window of trajectory_builder_3d.lua.  The reference computes the linear steps as
lround(linear_search_window / resolution) with the window a double and the resolution a float:
0.15 / 0.1f = 1.4999999776, one step, 27 translations -- not the 2 steps and 125 translations
0.15 / 0.10 suggests on paper.  The plan is pinned to what the formula gives (the single call, and
the reference, search that window); 125 x 343 = 42 875 candidates is the window of 0.2 m."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT, CERES, PLAN = "cmx_rt3d_match_grid_batch", "cmx_ceres3d_match_grids_batch", \
    "cmx_debug_rt3d_batch_plan"
HEADER = os.path.join(ROOT, "include", "cartographer_mi355x.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "cartographer_mi355x_debug.h")
LUA = (0.15, math.radians(1.0))


def _declaration(text, name):
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % name, stripped, re.S)
    assert m, f"{name} is not declared"
    return stripped, m


def test_header_declares_the_calls_and_lists_them():
    text = open(HEADER).read()
    for name in (RT, CERES):
        assert name in text.split("#ifndef")[0]                   # the entry-point list
        stripped, m = _declaration(text, name)
        assert len([a for a in m.group(1).split(",") if a.strip()]) == 9
    stripped, m = _declaration(text, RT)
    assert stripped.index("cmx_rt3d_match_grid(") < m.start() < stripped.index(
        "cmx_ceres3d_match_grids(")
    assert "cmx_ceres3d_match_grids_intensity stays a single" in text   # no batch form of it
    _, m = _declaration(open(DEBUG_HEADER).read(), PLAN)
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 6


def test_library_exports_the_calls_and_the_mirrors_have_their_argument_counts():
    from cartographer_amd import _lib
    L = _lib.lib()
    for name, count in ((RT, 9), (CERES, 9)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name), f"{name} is not exported"
        assert len(getattr(L, name).argtypes) == count
    assert PLAN in _lib.DEBUG_SYMBOLS
    assert len(getattr(L, PLAN).argtypes) == 6


def test_plan_struct_has_the_layout_a_c99_compiler_gives_it(tmp_path):
    import subprocess
    from cartographer_amd import _lib
    fields = [f[0] for f in _lib.DebugRt3DMatchPlan._fields_]
    src = tmp_path / "size.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cartographer_mi355x_debug.h"\n'
        'int main(void) {\n  printf("%zu", sizeof(cmx_debug_rt3d_match_plan));\n' +
        "".join(f'  printf(" %zu", offsetof(cmx_debug_rt3d_match_plan, {f}));\n' for f in fields) +
        '  return 0;\n}\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe])
    words = [int(w) for w in subprocess.run([exe], capture_output=True, text=True,
                                            check=True).stdout.split()]
    assert words[0] == C.sizeof(_lib.DebugRt3DMatchPlan)
    assert words[1:] == [getattr(_lib.DebugRt3DMatchPlan, f).offset for f in fields]


def test_python_mirror_has_the_entry_points():
    from cartographer_amd import scan_matching_3d as sm3
    assert list(inspect.signature(sm3.RealTimeCorrelativeScanMatcher3D.match_grid_batch)
                .parameters) == ["self", "initial_poses", "clouds", "grids"]
    assert list(inspect.signature(sm3.rt3d_batch_plan).parameters) == [
        "matcher", "resolutions", "num_points", "max_point_norms"]
    assert list(inspect.signature(sm3.ceres_match_grids_batch).parameters) == [
        "matcher", "target_translations", "initial_poses", "point_clouds_and_grids"]
    assert list(inspect.signature(sm3.CeresScanMatcher3D.match_grids_batch).parameters) == [
        "self", "target_translations", "initial_poses", "point_clouds_and_grids"]


def test_debug_switch_exists():
    from cartographer_amd import _lib
    try:
        _lib.debug_set(rt3d_batch_route=2)
    finally:
        _lib.debug_reset()


# ---- argument checks ------------------------------------------------------------------------
def _stand_in_grid(resolution=0.1, device=0):
    """Zeroed memory with the two members a check reads from a grid: its device and its
    resolution, the int and the float the handle begins with.  Its dims are 0: a grid nothing was
    inserted into, which no route looks into."""
    buffer = C.create_string_buffer(4096)
    C.c_int32.from_buffer(buffer).value = device
    C.c_float.from_buffer(buffer, 4).value = resolution
    return buffer


class _RtCall:
    """Four matches on stand-in grids: every check these tests reach is made before the device is
    touched."""

    def __init__(self, num=4, window=LUA):
        from cartographer_amd import _lib
        self.lib = _lib
        self.num = num
        self.options = _lib.RtOptions(window[0], window[1], 1e-1, 1e-1)
        self.stand_ins = [_stand_in_grid() for _ in range(num)]
        self.grids = (C.c_void_p * num)(*[C.addressof(b) for b in self.stand_ins])
        self.poses = (_lib.Pose3d * num)()
        for p in self.poses:
            p.q[0] = 1.0
        self.points = [np.full((3 + k, 3), 1.0 + k, np.float32) for k in range(num)]
        self.clouds = (C.c_void_p * num)(*[p.ctypes.data for p in self.points])
        self.counts = np.array([p.shape[0] for p in self.points], np.int32)
        self.scores = np.full(num, -7.0, np.float32)
        self.out = (_lib.Pose3d * num)()
        for p in self.out:
            p.t[0] = -7.0

    def __call__(self, **replace):
        a = dict(options=C.byref(self.options), grids=self.grids, num=self.num,
                 poses=C.cast(self.poses, C.c_void_p), clouds=self.clouds,
                 counts=self.counts.ctypes.data, scores=self.scores.ctypes.data,
                 out=C.cast(self.out, C.c_void_p), stats=None)
        a.update(replace)
        return self.lib.lib().cmx_rt3d_match_grid_batch(
            a["options"], a["grids"], a["num"], a["poses"], a["clouds"], a["counts"], a["scores"],
            a["out"], a["stats"])

    def error(self):
        return self.lib.lib().cmx_last_error().decode()

    def untouched(self):
        return bool(np.all(self.scores == -7.0)) and all(p.t[0] == -7.0 for p in self.out)


def test_rt_null_arrays_and_empty_lists_are_invalid():
    call = _RtCall()
    for name in ("options", "grids", "poses", "clouds", "counts", "scores", "out"):
        assert call(**{name: None}) == call.lib.INVALID_ARGUMENT, name
    assert call(num=0) == call.lib.INVALID_ARGUMENT
    assert "num_matches" in call.error()
    assert call(num=-2) == call.lib.INVALID_ARGUMENT
    assert call.untouched()


@pytest.mark.parametrize("index", [0, 2, 3])
def test_rt_every_rule_names_the_match_first_middle_and_last(index):
    def broken(change, word):
        call = _RtCall()
        change(call)
        assert call() == call.lib.INVALID_ARGUMENT
        assert f"match {index}" in call.error() and word in call.error(), call.error()
        assert call.untouched()

    def null_grid(call):
        call.grids[index] = None

    def null_cloud(call):
        call.clouds[index] = None

    def count(value):
        def change(call):
            call.counts[index] = value
        return change

    def fine_grid(call):
        # 0.15 m over a resolution of 0.1 mm: 1500 linear steps
        C.c_float.from_buffer(call.stand_ins[index], 4).value = 1e-4

    def other_device(call):
        C.c_int32.from_buffer(call.stand_ins[index]).value = 1

    broken(null_grid, "grid")
    broken(null_cloud, "cloud")
    broken(count(0), "point count")
    broken(count(-1), "point count")
    broken(count(2**24 + 1), "point count")
    broken(fine_grid, "search window")
    if index > 0:
        broken(other_device, "device")


def test_rt_one_pointer_with_two_counts_is_named():
    call = _RtCall()
    call.clouds[2] = call.clouds[3]
    assert call() == call.lib.INVALID_ARGUMENT
    assert "match 3" in call.error(), call.error()
    assert call.untouched()


def test_rt_windows_beyond_the_limits_are_refused_for_every_match():
    # L = 512 at the 0.1 m of the stand-ins; the last match is named when only its grid is coarse
    # enough for the others to pass
    call = _RtCall(window=(51.2, LUA[1]))
    assert call() == call.lib.INVALID_ARGUMENT
    assert "match 0" in call.error() and "search window" in call.error()
    call = _RtCall(window=(51.2, LUA[1]))
    for b in call.stand_ins[:3]:
        C.c_float.from_buffer(b, 4).value = 0.2
    assert call() == call.lib.INVALID_ARGUMENT
    assert "match 3" in call.error(), call.error()
    # fewer than 2^31 candidates: L = 100, A = 7 is 8.1e6 x 3375
    call = _RtCall(window=(10.0, 0.5))
    assert call() == call.lib.INVALID_ARGUMENT
    assert "match 0" in call.error() and "too large" in call.error(), call.error()


def test_rt_valid_arguments_reach_the_device():
    import torch
    call = _RtCall()
    status = call()
    if torch.cuda.is_available():
        assert status == call.lib.OK, call.error()
    else:
        assert status == call.lib.DEVICE_ERROR, call.error()
        assert call.untouched()


class _CeresCall:
    """Three matches of two pairs each on stand-in grids."""

    def __init__(self, num=3):
        from cartographer_amd import _lib
        self.lib = _lib
        self.num = num
        o = _lib.Ceres3DOptions()
        o.occupied_space_weight[0], o.occupied_space_weight[1] = 1.0, 6.0
        o.translation_weight, o.rotation_weight = 5.0, 4e2
        o.num_pairs, o.max_num_iterations = 2, 12
        self.options = o
        self.stand_ins = [_stand_in_grid(0.1 if k % 2 == 0 else 0.45) for k in range(2 * num)]
        self.grids = (C.c_void_p * (2 * num))(*[C.addressof(b) for b in self.stand_ins])
        self.targets = np.zeros((num, 3), np.float64)
        self.poses = (_lib.Pose3d * num)()
        for p in self.poses:
            p.q[0] = 1.0
        self.points = [np.full((2 + k, 3), 0.5 + k, np.float32) for k in range(2 * num)]
        self.clouds = (C.c_void_p * (2 * num))(*[p.ctypes.data for p in self.points])
        self.counts = np.array([p.shape[0] for p in self.points], np.int32)
        self.out = (_lib.Pose3d * num)()
        for p in self.out:
            p.t[0] = -7.0

    def __call__(self, **replace):
        a = dict(options=C.byref(self.options), num=self.num, targets=self.targets.ctypes.data,
                 poses=C.cast(self.poses, C.c_void_p), grids=self.grids, clouds=self.clouds,
                 counts=self.counts.ctypes.data, out=C.cast(self.out, C.c_void_p), summaries=None)
        a.update(replace)
        return self.lib.lib().cmx_ceres3d_match_grids_batch(
            a["options"], a["num"], a["targets"], a["poses"], a["grids"], a["clouds"], a["counts"],
            a["out"], a["summaries"])

    def error(self):
        return self.lib.lib().cmx_last_error().decode()

    def untouched(self):
        return all(p.t[0] == -7.0 for p in self.out)


def test_ceres_null_arrays_empty_lists_and_options_are_invalid():
    call = _CeresCall()
    for name in ("options", "targets", "poses", "grids", "clouds", "counts", "out"):
        assert call(**{name: None}) == call.lib.INVALID_ARGUMENT, name
    assert call(num=0) == call.lib.INVALID_ARGUMENT
    assert "num_matches" in call.error()
    call.options.num_pairs = 4
    assert call() == call.lib.INVALID_ARGUMENT
    assert call.untouched()


@pytest.mark.parametrize("index", [0, 1, 2])
def test_ceres_every_rule_names_the_match(index):
    def broken(change, word):
        call = _CeresCall()
        change(call, 2 * index + 1)
        assert call() == call.lib.INVALID_ARGUMENT
        assert f"match {index}" in call.error() and word in call.error(), call.error()
        assert call.untouched()

    def null_grid(call, at):
        call.grids[at] = None

    def null_cloud(call, at):
        call.clouds[at] = None

    def no_points(call, at):
        call.counts[at] = 0

    def other_device(call, at):
        C.c_int32.from_buffer(call.stand_ins[at]).value = 1

    def two_counts(call, at):
        call.clouds[at] = call.clouds[0]
        call.counts[0] = call.counts[at] + 1

    broken(null_grid, "grid")
    broken(null_cloud, "cloud")
    broken(no_points, "cloud")
    broken(other_device, "device")
    broken(two_counts, "cloud")


def test_ceres_valid_arguments_reach_the_device():
    import torch
    call = _CeresCall()
    status = call()
    if torch.cuda.is_available():
        assert status == call.lib.OK, call.error()
    else:
        assert status == call.lib.DEVICE_ERROR, call.error()
        assert call.untouched()


# ---- the plan -------------------------------------------------------------------------------
def _matcher(window=LUA):
    from cartographer_amd.scan_matching_3d import RealTimeCorrelativeScanMatcher3D
    return RealTimeCorrelativeScanMatcher3D(window[0], window[1], 1e-1, 1e-1)


def _plan(window, resolutions, num_points, norms):
    from cartographer_amd.scan_matching_3d import rt3d_batch_plan
    return rt3d_batch_plan(_matcher(window), resolutions, num_points, norms)


def _lround(x):
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def _window(window, resolution, max_norm):
    """BuildSearchSpace's formulas (GenerateExhaustiveSearchTransforms, SM3/
    real_time_correlative_scan_matcher_3d.cc:55-75) in numpy float32: L, A, T, R and the angular
    quotient before it is rounded."""
    f = np.float32
    res = f(resolution)
    L = _lround(window[0] / float(res))                  # double / float -> double
    rng = max(f(max_norm), f(3) * res)
    step = (f(1) - f(1e-3)) * np.arccos(f(1) - (res * (res * f(1))) / (f(2) * (rng * (rng * f(1)))))
    assert step.dtype == np.float32
    quotient = window[1] / float(step)
    A = _lround(quotient)
    return (L, A, (2 * L + 1) ** 3, (2 * A + 1) ** 3), quotient


def test_plan_gives_the_window_of_the_formulas():
    rng = np.random.default_rng(5)
    checked = 0
    for window in [LUA, (0.2, math.radians(1.0)), (0.5, 0.02), (0.05, 0.004), (1.0, 0.01)]:
        resolutions = rng.choice([0.05, 0.1, 0.2, 0.45], 12)
        norms = rng.uniform(0.05, 20.0, 12)
        counts = rng.integers(1, 500, 12)
        plans = _plan(window, resolutions, counts, norms)
        for p, res, norm in zip(plans, resolutions, norms):
            expected, quotient = _window(window, res, norm)
            # (numpy's arccos may differ from libm's in the last place: a quotient that close to a
            # half step says nothing)
            if abs(quotient % 1 - 0.5) < 1e-3 or abs((window[0] / res) % 1 - 0.5) < 1e-6:
                continue
            assert (p["L"], p["A"], p["T"], p["R"]) == expected, (window, res, norm, p)
            checked += 1
    assert checked >= 50


def test_plan_of_the_lua_default():
    """0.15 m / 1 degree at 0.10 m and a 15 m range: the double 0.15 over the float 0.1f is
    1.4999999776, ONE linear step (module docstring); 2.62 angular steps round to 3."""
    assert 0.15 / float(np.float32(0.1)) < 1.5
    (p,) = _plan(LUA, [0.1], [300], [15.0])
    assert (p["L"], p["A"], p["T"], p["R"]) == (1, 3, 27, 343)
    assert (p["L"], p["A"], p["T"], p["R"]) == _window(LUA, 0.1, 15.0)[0]
    assert p["route"] == 0 and p["set"] == 0 and p["first_block"] == 0
    assert p["blocks"] == 343 * 1                        # ceil(27 / 64) blocks per rotation
    # two linear steps, the 125 x 343 = 42 875 candidates, are the window of 0.2 m
    (p,) = _plan((0.2, LUA[1]), [0.1], [300], [15.0])
    assert (p["L"], p["A"], p["T"], p["R"]) == (2, 3, 125, 343)
    assert p["blocks"] == 343 * 2


def test_plan_of_a_single_candidate():
    (p,) = _plan((0.04, 1e-4), [0.1], [10], [5.0])
    assert (p["L"], p["A"], p["T"], p["R"], p["blocks"]) == (0, 0, 1, 1, 1)
    # ... next to a normal match: consecutive blocks of one set
    a, b, c = _plan((0.04, math.radians(1.0)), [0.1, 0.1, 0.1], [10, 10, 10], [15.0, 0.1, 15.0])
    assert (b["L"], b["A"], b["R"]) == (0, 0, 1)         # a 0.3 m range: a step of 19 degrees
    assert (a["set"], b["set"], c["set"]) == (0, 0, 0)
    assert (a["first_block"], b["first_block"], c["first_block"]) == (0, 343, 344)


@pytest.mark.parametrize("window,word", [((51.2, 0.01), "unsupported"), ((0.1, 1.0), "unsupported"),
                                         ((10.0, 0.015), "too large")])
def test_plan_refuses_a_window_beyond_the_limits(window, word):
    from cartographer_amd import _lib
    with pytest.raises(_lib.CmxError) as e:
        _plan(window, [0.2, 0.1], [10, 10], [1.0, 20.0])
    assert e.value.status == _lib.INVALID_ARGUMENT
    assert "match" in str(e.value) and word in str(e.value)


def test_route_follows_the_work_and_flips_under_the_switch():
    from cartographer_amd import _lib
    # lua window: 9 261 candidates; 300 points are 2.8e6 lookups, 2^24 points 1.6e11
    args = (LUA, [0.1, 0.1, 0.1], [300, 2**24, 300], [15.0, 15.0, float("nan")])
    try:
        plans = _plan(*args)
        assert [p["route"] for p in plans] == [0, 1, 1]  # by size; a non-finite cloud is single
        assert [p["set"] for p in plans] == [0, -1, -1]
        assert plans[1]["blocks"] == 0
        _lib.debug_set(rt3d_batch_route=1)
        plans = _plan(*args)
        assert [p["route"] for p in plans] == [0, 0, 1]
        # (200 MB of points: past the staging bound of a set, so a set of its own)
        assert (plans[1]["set"], plans[1]["first_block"], plans[1]["blocks"]) == (1, 0, 343)
        _lib.debug_set(rt3d_batch_route=2)
        assert [p["route"] for p in _plan(*args)] == [1, 1, 1]
    finally:
        _lib.debug_reset()
