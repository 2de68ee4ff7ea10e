"""CPU-side checks of cmx_fast2d_create_batch (the matchers of many submaps in one call):
declared, exported, mirrored with the header's argument count and struct size, every argument
check made before the device is touched -- with the index of the failing source in
cmx_last_error and every out[k] NULL -- no CPU fallback, and ConstraintBuilder2D(batch_create=True)
deferring the construction of its matchers to the flush."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cmx_fast2d_create_batch"
HEADER = os.path.join(ROOT, "include", "cartographer_mi355x.h")


def _header():
    return open(HEADER).read()


def test_header_declares_the_call_and_lists_it():
    text = _header()
    assert NAME in text.split("#ifndef")[0]                       # the entry-point list
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % NAME, stripped, re.S)
    assert m, "not declared"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 5


def test_library_exports_the_call_and_the_mirror_has_its_argument_count():
    from cartographer_amd import _lib
    L = _lib.lib()
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert hasattr(L, NAME), f"{NAME} is not exported"
    assert len(getattr(L, NAME).argtypes) == 5


def test_source_struct_has_the_size_a_c99_compiler_gives_it(tmp_path):
    """sizeof and member offsets of cmx_fast2d_source from a C99 program against the ctypes
    mirror; compiling it -pedantic -Werror is also the check that the header is still plain C."""
    from cartographer_amd import _lib
    fields = [f[0] for f in _lib.Fast2DSource._fields_]
    assert fields == ["limits", "cells", "grid", "tsdf"]
    src = tmp_path / "size.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cartographer_mi355x.h"\n'
        'int main(void) {\n  printf("%zu", sizeof(cmx_fast2d_source));\n' +
        "".join(f'  printf(" %zu", offsetof(cmx_fast2d_source, {f}));\n' for f in fields) +
        '  return 0;\n}\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe])
    words = [int(w) for w in subprocess.run([exe], capture_output=True, text=True,
                                            check=True).stdout.split()]
    assert words[0] == C.sizeof(_lib.Fast2DSource)
    assert words[1:] == [getattr(_lib.Fast2DSource, f).offset for f in fields]


def test_python_mirror_has_the_entry_points():
    import inspect
    from cartographer_amd import constraint_builder, scan_matching
    assert list(inspect.signature(
        scan_matching.FastCorrelativeScanMatcher2D.create_batch).parameters) == [
            "grids", "branch_and_bound_depth", "linear_search_window", "angular_search_window",
            "device"]
    parameter = inspect.signature(
        constraint_builder.ConstraintBuilder2D.__init__).parameters["batch_create"]
    assert parameter.default is False


def test_debug_switch_exists():
    from cartographer_amd import _lib
    try:
        _lib.debug_set(fast2d_create_chain=2)
    finally:
        _lib.debug_reset()


# ---- argument checks ------------------------------------------------------------------------
class _Call:
    """Four host-cell sources (4 x 3 cells, the probability range) and everything a call needs;
    tests damage one piece and call."""

    def __init__(self, num=4):
        from cartographer_amd import _lib
        self.lib = _lib
        self.num = num
        self.options = _lib.Fast2DOptions(7.0, 0.5, 3)
        self.limits = [_lib.Grid2DLimits(0.05, 1.0, 1.0, 4, 3, 0.1, 0.9) for _ in range(num)]
        self.cells = [np.full(12, 1000 + k, np.uint16) for k in range(num)]
        self.sources = (_lib.Fast2DSource * num)()
        for k in range(num):
            self.sources[k].limits = C.pointer(self.limits[k])
            self.sources[k].cells = self.cells[k].ctypes.data
        self.out = (C.c_void_p * num)(*([0xdead] * num))           # must come back NULL

    def __call__(self, options="own", sources="own", num=None, out="own"):
        L = self.lib.lib()
        return L.cmx_fast2d_create_batch(
            C.byref(self.options) if options == "own" else options,
            self.sources if sources == "own" else sources,
            self.num if num is None else num, 0, self.out if out == "own" else out)

    def error(self):
        return self.lib.lib().cmx_last_error().decode()

    def assert_invalid(self, status, index=None):
        assert status == self.lib.INVALID_ARGUMENT, self.error()
        assert all(h is None for h in self.out), list(self.out)
        if index is not None:
            assert f"source {index}" in self.error(), self.error()


def test_null_arguments_are_invalid():
    call = _Call()
    call.assert_invalid(call(options=None))
    call = _Call()
    call.assert_invalid(call(sources=None))
    call = _Call()
    assert call(out=None) == call.lib.INVALID_ARGUMENT


def test_no_sources_is_invalid():
    call = _Call()
    assert call(num=0) == call.lib.INVALID_ARGUMENT
    assert "num_sources" in call.error()
    call = _Call()
    assert call(num=-3) == call.lib.INVALID_ARGUMENT


def test_a_source_needs_exactly_one_kind():
    call = _Call()
    call.sources[1].limits = None
    call.sources[1].cells = None
    call.assert_invalid(call(), index=1)
    assert "no kind" in call.error()
    call = _Call()
    call.sources[3].grid = 0x1000            # never dereferenced: the count of kinds comes first
    call.assert_invalid(call(), index=3)
    assert "more than one kind" in call.error()
    call = _Call()
    call.sources[0].limits = None
    call.sources[0].cells = None
    call.sources[0].grid = 0x1000
    call.sources[0].tsdf = 0x1000
    call.assert_invalid(call(), index=0)


@pytest.mark.parametrize("fault", ["max_cost_above_one", "no_cells", "no_rows", "null_cells",
                                   "null_limits", "inverted_range", "resolution", "too_large"])
def test_a_bad_source_in_third_place_is_named(fault):
    """Every argument check of cmx_fast2d_create, made for a source in the middle of the list:
    CMX_INVALID_ARGUMENT with the index, nothing built (no device is needed to get there)."""
    call = _Call()
    lim = call.limits[2]
    if fault == "max_cost_above_one":
        lim.min_correspondence_cost, lim.max_correspondence_cost = -1.5, 1.5
    elif fault == "no_cells":
        lim.num_x_cells = 0
    elif fault == "no_rows":
        lim.num_y_cells = 0
    elif fault == "null_cells":
        call.sources[2].cells = None
    elif fault == "null_limits":
        call.sources[2].limits = None
    elif fault == "inverted_range":
        lim.min_correspondence_cost, lim.max_correspondence_cost = 0.9, 0.1
    elif fault == "resolution":
        lim.resolution = 0.0
    elif fault == "too_large":
        lim.num_x_cells = 16385
    call.assert_invalid(call(), index=2)


@pytest.mark.parametrize("depth", [0, 13])
def test_a_bad_depth_is_invalid(depth):
    """The options hold for every source: the first one is named."""
    call = _Call()
    call.options.branch_and_bound_depth = depth
    call.assert_invalid(call(), index=0)
    assert "branch_and_bound_depth" in call.error()


def test_no_cpu_fallback_without_device():
    call = _Call()
    if call.lib.lib().cmx_device_count() > 0:
        pytest.skip("a HIP device is present")
    assert call() == call.lib.DEVICE_ERROR
    assert "no CPU fallback" in call.error()
    assert all(h is None for h in call.out)
    from cartographer_amd import scan_matching as sm
    grid = sm.Grid2D(np.zeros((4, 4), np.uint16), 0.05, 0.1, 0.1)
    with pytest.raises(call.lib.CmxError) as e:
        sm.FastCorrelativeScanMatcher2D.create_batch([grid, grid], 3)
    assert e.value.status == call.lib.DEVICE_ERROR


# ---- ConstraintBuilder2D(batch_create=True) ------------------------------------------------
def test_builder_defers_construction_to_one_create_batch_call(monkeypatch):
    """With batch_create nothing is built when pairs are added; the flush asks for all missing
    matchers -- each submap once -- in ONE create_batch call before the searches.  create_batch
    and the search are replaced: no device is touched."""
    from cartographer_amd import constraint_builder as cb, scan_matching as sm
    calls = []

    class FakeMatcher:
        def __init__(self, grid):
            self.grid = grid

    def fake_create_batch(grids, depth, linear, angular, device=0):
        calls.append((list(grids), depth, linear, angular, device))
        return [FakeMatcher(g) for g in grids]

    def no_single_create(*args, **kwargs):
        raise AssertionError("batch_create must not build a matcher on its own")

    searched = []

    def fake_match_group(self, xyz, items):
        assert all(isinstance(i.matcher, FakeMatcher) for i in items)
        assert all(i.matcher.grid is i.submap.grid for i in items)
        searched.append([i.submap_id for i in items])

    monkeypatch.setattr(sm.FastCorrelativeScanMatcher2D, "create_batch",
                        staticmethod(fake_create_batch))
    monkeypatch.setattr(sm.FastCorrelativeScanMatcher2D, "__init__", no_single_create)
    monkeypatch.setattr(cb.ConstraintBuilder2D, "_match_group", fake_match_group)

    options = cb.ConstraintBuilderOptions(sampling_ratio=1.0, branch_and_bound_depth=4)
    builder = cb.ConstraintBuilder2D(options, device=0, batch_create=True)
    grids = [sm.Grid2D(np.zeros((4, 4), np.uint16), 0.05, 0.1, 0.1) for _ in range(3)]
    submaps = [cb.Submap2D(sm.Rigid2d(), g) for g in grids]
    cloud = np.zeros((5, 3), np.float32)
    for k in range(3):
        builder.maybe_add_global_constraint((0, k), submaps[k], (0, 7), cloud)
    builder.maybe_add_constraint((0, 1), submaps[1], (0, 7), cloud, sm.Rigid2d(0.1, 0.0, 0.0))
    assert calls == [] and builder.num_scan_matchers() == 3
    builder.notify_end_of_node()
    assert len(calls) == 1
    assert [id(g) for g in calls[0][0]] == [id(g) for g in grids]      # each submap once
    assert calls[0][1:] == (4, options.linear_search_window, options.angular_search_window, 0)
    assert searched == [[(0, 0), (0, 1), (0, 2), (0, 1)]]
    # the matchers stay: a second node builds nothing
    builder.maybe_add_global_constraint((0, 2), submaps[2], (0, 8), cloud)
    builder.notify_end_of_node()
    assert len(calls) == 1 and builder.num_scan_matchers() == 3
    # a deleted one is built again, alone
    builder.delete_scan_matcher((0, 0))
    builder.maybe_add_global_constraint((0, 0), submaps[0], (0, 9), cloud)
    builder.notify_end_of_node()
    assert len(calls) == 2 and [id(g) for g in calls[1][0]] == [id(grids[0])]
