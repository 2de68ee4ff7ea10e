"""CPU-side checks of cmx_fast3d_match_pairs / cmx_fast3d_refine_pairs (many nodes against
submaps in one fast-3D batch): declared, exported, mirrored with the header's argument counts,
and -- like everything else here -- without a CPU fallback."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmx_fast3d_match_pairs", "cmx_fast3d_refine_pairs")


def _declarations():
    """name -> number of parameters, from the header (comments stripped)."""
    text = open(os.path.join(ROOT, "include", "cartographer_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name in NAMES:
        m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % name, text, re.S)
        if m:
            out[name] = len([a for a in m.group(1).split(",") if a.strip()])
    return out


def test_header_declares_both_calls():
    assert _declarations() == {"cmx_fast3d_match_pairs": 10, "cmx_fast3d_refine_pairs": 8}


def test_library_exports_both_calls():
    from cartographer_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name), f"{name} is not exported"


def test_python_prototypes_have_the_header_argument_counts():
    from cartographer_amd import _lib
    L = _lib.lib()
    for name, count in _declarations().items():
        assert len(getattr(L, name).argtypes) == count, name


def test_no_cpu_fallback_without_device():
    from cartographer_amd import _lib
    L = _lib.lib()
    if L.cmx_device_count() > 0:
        pytest.skip("a HIP device is present")
    handles = (C.c_void_p * 1)(None)
    data = (C.POINTER(_lib.NodeData3D) * 1)(C.pointer(_lib.NodeData3D()))
    poses = (_lib.Pose3d * 1)()
    full = (C.c_int32 * 1)(0)
    thresholds = (C.c_float * 1)(0.5)
    found = (C.c_int32 * 1)(0)
    results = (_lib.Result3D * 1)()
    stats = _lib.MatchStats()
    status = L.cmx_fast3d_match_pairs(handles, 1, C.cast(poses, C.c_void_p),
                                      C.cast(poses, C.c_void_p), C.cast(full, C.c_void_p),
                                      C.cast(thresholds, C.c_void_p), data,
                                      C.cast(found, C.c_void_p), C.cast(results, C.c_void_p),
                                      C.byref(stats))
    assert status == _lib.DEVICE_ERROR
    assert b"no CPU fallback" in L.cmx_last_error()
    options = _lib.Ceres3DOptions()
    out = (_lib.Pose3d * 1)()
    status = L.cmx_fast3d_refine_pairs(C.byref(options), handles, 1, C.cast(found, C.c_void_p),
                                       C.cast(poses, C.c_void_p), data,
                                       C.cast(out, C.c_void_p), None)
    assert status == _lib.DEVICE_ERROR
    assert b"no CPU fallback" in L.cmx_last_error()
