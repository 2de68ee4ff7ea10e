"""CPU-side checks of the five calls for lists of (node, submap) pairs in 2D
(cmx_fast2d_match_pairs[_resident], cmx_fast2d_refine_pairs[_resident],
cmx_ceres2d_refine_pairs_tsdf): declared, exported, mirrored with the header's argument counts,
and -- like everything else here -- without a CPU fallback."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"cmx_fast2d_match_pairs": 11, "cmx_fast2d_match_pairs_resident": 10,
          "cmx_fast2d_refine_pairs": 9, "cmx_fast2d_refine_pairs_resident": 8,
          "cmx_ceres2d_refine_pairs_tsdf": 9}


def _declarations():
    """name -> number of parameters, from the header (comments stripped)."""
    text = open(os.path.join(ROOT, "include", "cartographer_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name in COUNTS:
        m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % name, text, re.S)
        if m:
            out[name] = len([a for a in m.group(1).split(",") if a.strip()])
    return out


def test_header_declares_the_five_calls():
    assert _declarations() == COUNTS


def test_library_exports_the_five_calls():
    from cartographer_amd import _lib
    L = _lib.lib()
    for name in COUNTS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name), f"{name} is not exported"


def test_python_prototypes_have_the_header_argument_counts():
    from cartographer_amd import _lib
    L = _lib.lib()
    for name, count in COUNTS.items():
        assert len(getattr(L, name).argtypes) == count, name


def test_python_mirror_has_the_entry_points():
    import inspect
    from cartographer_amd import constraint_builder, scan_matching
    assert list(inspect.signature(scan_matching.match_pairs).parameters) == [
        "matchers", "initial_pose_estimates", "match_full_submap", "min_scores", "point_clouds"]
    assert hasattr(scan_matching.CeresScanMatcher2D, "refine_pairs")
    assert hasattr(scan_matching.CeresScanMatcher2D, "refine_pairs_tsdf")
    pairs = inspect.signature(constraint_builder.ConstraintBuilder2D.__init__).parameters["pairs"]
    assert pairs.default is False


def test_no_cpu_fallback_without_device():
    from cartographer_amd import _lib
    L = _lib.lib()
    if L.cmx_device_count() > 0:
        pytest.skip("a HIP device is present")
    handles = (C.c_void_p * 1)(None)
    cloud = (C.c_float * 3)(1.0, 0.0, 0.0)
    clouds = (C.c_void_p * 1)(C.addressof(cloud))
    counts = (C.c_int32 * 1)(1)
    poses = (_lib.Pose2d * 1)()
    out = (_lib.Pose2d * 1)()
    full = (C.c_int32 * 1)(0)
    thresholds = (C.c_float * 1)(0.5)
    found = (C.c_int32 * 1)(0)
    scores = (C.c_float * 1)(0.0)
    stats = _lib.MatchStats()
    options = _lib.Ceres2DOptions(1.0, 1.0, 1.0, 0, 10)
    p = lambda a: C.cast(a, C.c_void_p)   # noqa: E731
    calls = [
        lambda: L.cmx_fast2d_match_pairs(handles, 1, p(poses), p(full), p(thresholds), clouds,
                                         p(counts), p(found), p(scores), p(out), C.byref(stats)),
        lambda: L.cmx_fast2d_match_pairs_resident(handles, 1, p(poses), p(full), p(thresholds),
                                                  handles, p(found), p(scores), p(out),
                                                  C.byref(stats)),
        lambda: L.cmx_fast2d_refine_pairs(C.byref(options), handles, 1, p(found), p(poses), clouds,
                                          p(counts), p(out), None),
        lambda: L.cmx_fast2d_refine_pairs_resident(C.byref(options), handles, 1, p(found),
                                                   p(poses), handles, p(out), None),
        lambda: L.cmx_ceres2d_refine_pairs_tsdf(C.byref(options), handles, 1, p(found), p(poses),
                                                clouds, p(counts), p(out), None),
        # whatever the arguments: nothing at all
        lambda: L.cmx_fast2d_match_pairs(None, 0, None, None, None, None, None, None, None, None,
                                         None),
        lambda: L.cmx_fast2d_refine_pairs(None, None, 0, None, None, None, None, None, None),
    ]
    for call in calls:
        assert call() == _lib.DEVICE_ERROR
        assert b"no CPU fallback" in L.cmx_last_error()
