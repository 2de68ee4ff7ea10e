"""CPU-side checks of cmx_fast3d_create_batch (the fast-3D matchers of many submaps in one call):
declared, exported, mirrored with the header's argument count and struct layout, every argument
check made before the device is touched -- with the index of the failing source in
cmx_last_error and every out[k] NULL -- and ConstraintBuilder3D: unchanged without batch_create,
deferring the construction of its matchers to the flush with it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cmx_fast3d_create_batch"
HEADER = os.path.join(ROOT, "include", "cartographer_mi355x.h")
FIELDS = ["resolution", "grid_size", "voxels", "num_voxels", "low_resolution",
          "low_resolution_voxels", "num_low_resolution_voxels", "high_resolution_grid",
          "low_resolution_grid", "rotational_scan_matcher_histogram", "histogram_size"]


def test_header_declares_the_call_and_lists_it():
    text = open(HEADER).read()
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


def test_source_struct_has_the_layout_a_c99_compiler_gives_it(tmp_path):
    """sizeof and member offsets of cmx_fast3d_source from a C99 program against the ctypes
    mirror; compiling it -pedantic -Werror is also the check that the header is still plain C."""
    from cartographer_amd import _lib
    assert [f[0] for f in _lib.Fast3DSource._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cartographer_mi355x.h"\n'
        'int main(void) {\n  printf("%zu", sizeof(cmx_fast3d_source));\n' +
        "".join(f'  printf(" %zu", offsetof(cmx_fast3d_source, {f}));\n' for f in FIELDS) +
        '  return 0;\n}\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe])
    words = [int(w) for w in subprocess.run([exe], capture_output=True, text=True,
                                            check=True).stdout.split()]
    assert words[0] == C.sizeof(_lib.Fast3DSource)
    assert words[1:] == [getattr(_lib.Fast3DSource, f).offset for f in FIELDS]


def test_python_mirror_has_the_entry_points():
    import inspect
    from cartographer_amd import constraint_builder, scan_matching_3d
    parameters = inspect.signature(scan_matching_3d.fast3d_create_batch).parameters
    assert list(parameters) == ["sources", "device", "options"]
    assert parameters["device"].default == 0
    assert parameters["options"].kind is inspect.Parameter.VAR_KEYWORD
    parameter = inspect.signature(
        constraint_builder.ConstraintBuilder3D.__init__).parameters["batch_create"]
    assert parameter.default is False
    with pytest.raises(TypeError):
        scan_matching_3d.fast3d_create_batch([], no_such_option=1)


def test_debug_switch_exists():
    from cartographer_amd import _lib
    try:
        _lib.debug_set(fast3d_create_chain=2)
    finally:
        _lib.debug_reset()


# ---- argument checks ------------------------------------------------------------------------
class _Call:
    """Four voxel-list sources (a few voxels around the origin, a histogram of 8 bins) and
    everything a call needs; tests damage one piece and call."""

    def __init__(self, num=4):
        from cartographer_amd import _lib
        self.lib = _lib
        self.num = num
        self.options = _lib.Fast3DOptions(4, 2, 0.77, 0.55, 5.0, 1.0, 0.26)
        self.voxels, self.low, self.hist = [], [], []
        self.sources = (_lib.Fast3DSource * num)()
        for k in range(num):
            vox = np.zeros(3, _lib.VOXEL_DTYPE)
            vox["x"], vox["y"], vox["z"] = [-2, 0, 5 + k], [1, -3, 2], [0, 1, -1]
            vox["value"] = 20000 + k
            low = vox[:2].copy()
            hist = np.full(8, 1.0 + k, np.float32)
            self.voxels.append(vox)
            self.low.append(low)
            self.hist.append(hist)
            s = self.sources[k]
            s.resolution, s.grid_size = 0.1, 128
            s.voxels, s.num_voxels = vox.ctypes.data, 3
            s.low_resolution = 0.45
            s.low_resolution_voxels, s.num_low_resolution_voxels = low.ctypes.data, 2
            s.rotational_scan_matcher_histogram, s.histogram_size = hist.ctypes.data, 8
        self.out = (C.c_void_p * num)(*([0xdead] * num))           # must come back NULL

    def __call__(self, options="own", sources="own", num=None, out="own"):
        L = self.lib.lib()
        return L.cmx_fast3d_create_batch(
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


@pytest.mark.parametrize("depth,frd,word", [(0, 2, "branch_and_bound_depth"),
                                            (13, 2, "branch_and_bound_depth"),
                                            (4, 0, "full_resolution_depth")])
def test_bad_options_are_invalid(depth, frd, word):
    """The options hold for every source; nothing is built."""
    call = _Call()
    call.options.branch_and_bound_depth = depth
    call.options.full_resolution_depth = frd
    call.assert_invalid(call())
    assert word in call.error()


@pytest.mark.parametrize("fault", ["resolution", "low_resolution", "grid_size", "histogram_size",
                                   "null_histogram", "null_voxels", "null_low_voxels",
                                   "negative_count", "both_kinds", "nothing_set"])
def test_a_bad_source_in_third_place_is_named(fault):
    """Every argument check of cmx_fast3d_create, made for a source in the middle of the list:
    CMX_INVALID_ARGUMENT with the index, nothing built (no device is needed to get there)."""
    call = _Call()
    s = call.sources[2]
    if fault == "resolution":
        s.resolution = 0.0
    elif fault == "low_resolution":
        s.low_resolution = -0.45
    elif fault == "grid_size":
        call.voxels[2]["x"][2] = 64                  # needs grid_size 256
    elif fault == "histogram_size":
        s.histogram_size = -1
    elif fault == "null_histogram":
        s.rotational_scan_matcher_histogram = None
    elif fault == "null_voxels":
        s.voxels = None
    elif fault == "null_low_voxels":
        s.low_resolution_voxels = None
    elif fault == "negative_count":
        s.num_voxels = -1
    elif fault == "both_kinds":
        s.low_resolution_grid = 0x1000               # never dereferenced: the kinds come first
    elif fault == "nothing_set":
        C.memset(C.byref(s), 0, C.sizeof(s))
    call.assert_invalid(call(), index=2)
    if fault == "grid_size":
        assert "grid_size 128" in call.error()
    if fault == "both_kinds":
        assert "more than one kind" in call.error()


def test_good_sources_reach_the_device():
    """The same four sources undamaged: the call gets as far as the device (and fails loudly
    where there is none: no CPU fallback)."""
    call = _Call()
    status = call()
    if call.lib.lib().cmx_device_count() > 0:
        assert status == call.lib.OK, call.error()
        for h in call.out:
            call.lib.lib().cmx_fast3d_destroy(h)
        return
    assert status == call.lib.DEVICE_ERROR
    assert all(h is None for h in call.out)


# ---- ConstraintBuilder3D --------------------------------------------------------------------
def _builder_fixture(monkeypatch, batch_create):
    from cartographer_amd import constraint_builder as cb, scan_matching_3d as sm3
    log = dict(single=[], batch=[], searched=[])

    class FakeMatcher:
        def __init__(self, *args, **kwargs):
            self.args, self.kwargs = args, kwargs
            log["single"].append(self)

    def fake_create_batch(sources, *, device=0, **options):
        sources = list(sources)
        log["batch"].append((sources, device, options))
        made = []
        for source in sources:
            m = object.__new__(FakeMatcher)
            m.args, m.kwargs = tuple(source), dict(options, device=device)
            made.append(m)
        return made

    def fake_match_pairs(matchers, node_poses, submap_poses, full, min_scores, datas):
        assert all(isinstance(m, FakeMatcher) for m in matchers)
        log["searched"].append(list(matchers))
        return [None] * len(matchers), {}

    monkeypatch.setattr(sm3, "FastCorrelativeScanMatcher3D", FakeMatcher)
    monkeypatch.setattr(sm3, "fast3d_create_batch", fake_create_batch)
    monkeypatch.setattr(sm3, "fast3d_match_pairs", fake_match_pairs)
    options = cb.ConstraintBuilderOptions3D(sampling_ratio=1.0, branch_and_bound_depth=5,
                                            full_resolution_depth=2)
    builder = cb.ConstraintBuilder3D(options, device=0, batch_create=batch_create) \
        if batch_create is not None else cb.ConstraintBuilder3D(options, device=0)
    none = np.zeros(0, sm3.VOXEL_DTYPE)
    submaps = [cb.Submap3D(0.1, none, 128, 0.45, none, np.full(4, float(k), np.float32))
               for k in range(3)]
    data = sm3.TrajectoryNodeData(np.zeros((4, 3), np.float32), np.zeros((2, 3), np.float32),
                                  np.ones(4, np.float32))
    return cb, sm3, builder, submaps, data, log


def _expected_arguments(submap):
    return (submap.high_resolution, submap.high_resolution_voxels, submap.grid_size,
            submap.low_resolution, submap.low_resolution_voxels,
            submap.rotational_scan_matcher_histogram)


def _expected_options(options):
    return dict(branch_and_bound_depth=options.branch_and_bound_depth,
                full_resolution_depth=options.full_resolution_depth,
                min_rotational_score=options.min_rotational_score,
                min_low_resolution_score=options.min_low_resolution_score,
                linear_xy_search_window=options.linear_xy_search_window,
                linear_z_search_window=options.linear_z_search_window,
                angular_search_window=options.angular_search_window, device=0)


@pytest.mark.parametrize("batch_create", [None, False])
def test_builder_without_batch_create_is_unchanged(monkeypatch, batch_create):
    """One constructor per new SubmapId when its first pair is added, with the arguments it
    always had; the matcher travels with the pair; no create_batch call."""
    cb, sm3, builder, submaps, data, log = _builder_fixture(monkeypatch, batch_create)
    rotation = (1.0, 0.0, 0.0, 0.0)
    for k in range(3):
        builder.maybe_add_global_constraint((0, k), submaps[k], (0, 7), data, rotation, rotation)
        assert len(log["single"]) == k + 1 and builder.num_scan_matchers() == k + 1
    builder.maybe_add_constraint((0, 1), submaps[1], (0, 7), data, sm3.Rigid3d(), sm3.Rigid3d())
    assert len(log["single"]) == 3
    for k, m in enumerate(log["single"]):
        assert all(a is b for a, b in zip(m.args, _expected_arguments(submaps[k])))
        assert m.kwargs == _expected_options(builder.options)
    builder.delete_scan_matcher((0, 0))               # the pending pair keeps its matcher
    builder.notify_end_of_node()
    assert log["batch"] == []
    assert log["searched"] == [[log["single"][k] for k in (0, 1, 2, 1)]]
    assert builder.num_scan_matchers() == 2


def test_builder_defers_construction_to_one_create_batch_call(monkeypatch):
    """With batch_create nothing is built when pairs are added; the flush asks for all missing
    matchers -- each submap once -- in ONE create_batch call before the searches."""
    cb, sm3, builder, submaps, data, log = _builder_fixture(monkeypatch, True)
    rotation = (1.0, 0.0, 0.0, 0.0)
    for k in range(3):
        builder.maybe_add_global_constraint((0, k), submaps[k], (0, 7), data, rotation, rotation)
    builder.maybe_add_constraint((0, 1), submaps[1], (0, 7), data, sm3.Rigid3d(), sm3.Rigid3d())
    assert log["batch"] == [] and log["single"] == [] and builder.num_scan_matchers() == 0
    builder.notify_end_of_node()
    assert len(log["batch"]) == 1 and log["single"] == []
    sources, device, options = log["batch"][0]
    assert len(sources) == 3 and device == 0
    for k, source in enumerate(sources):                               # each submap once
        assert all(a is b for a, b in zip(source, _expected_arguments(submaps[k])))
    assert dict(options, device=0) == _expected_options(builder.options)
    assert builder.num_scan_matchers() == 3
    (searched,) = log["searched"]
    assert [m.args[5][0] for m in searched] == [0.0, 1.0, 2.0, 1.0]
    assert searched[1] is searched[3]
    # the matchers stay: a second node builds nothing
    builder.maybe_add_global_constraint((0, 2), submaps[2], (0, 8), data, rotation, rotation)
    builder.notify_end_of_node()
    assert len(log["batch"]) == 1 and builder.num_scan_matchers() == 3
    # a deleted one is built again, alone
    builder.delete_scan_matcher((0, 0))
    builder.maybe_add_global_constraint((0, 0), submaps[0], (0, 9), data, rotation, rotation)
    builder.notify_end_of_node()
    assert len(log["batch"]) == 2 and len(log["batch"][1][0]) == 1
    assert builder.num_scan_matchers() == 3
    # deleted between enqueue and flush: the pending pair still gets a matcher, the builder
    # keeps none for the submap
    builder.delete_scan_matcher((0, 1))
    builder.maybe_add_global_constraint((0, 1), submaps[1], (0, 10), data, rotation, rotation)
    builder.delete_scan_matcher((0, 1))
    builder.notify_end_of_node()
    assert len(log["batch"]) == 3 and len(log["searched"][-1]) == 1
    assert builder.num_scan_matchers() == 2
