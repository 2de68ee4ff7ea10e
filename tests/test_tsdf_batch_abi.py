"""C ABI of the batched real-time matcher on resident TSDF2Ds (CPU): both entries are declared
in the header and exported by the library, their argument checks come before the device, and
there is no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cmx_rt2d_match_tsdf_grid_batch", "cmx_rt2d_match_tsdf_grid_batch_resident")


def test_both_entries_are_declared_and_exported():
    from cartographer_amd import _lib
    header = open(os.path.join(ROOT, "include", "cartographer_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"cmx_status\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None
    for switch in ("rt2d_tsdf_batch_legacy", "rt2d_tsdf_batch_bulk", "rt2d_tsdf_verify"):
        _lib.debug_set(**{switch: 1})
    _lib.debug_reset()


def test_argument_checks_come_before_the_device():
    from cartographer_amd import _lib
    L = _lib.lib()
    opts = _lib.RtOptions(0.3, 0.1, 0.1, 0.1)
    one = (C.c_void_p * 1)(None)
    poses = np.zeros(3, np.float64)
    scores = np.zeros(1, np.float64)
    cloud = np.zeros((4, 3), np.float32)
    clouds = (C.c_void_p * 1)(cloud.ctypes.data)
    counts = np.array([4], np.int32)
    stats = _lib.MatchStats()
    host = L.cmx_rt2d_match_tsdf_grid_batch
    resident = L.cmx_rt2d_match_tsdf_grid_batch_resident
    good = (C.byref(opts), one, 1, poses.ctypes.data, clouds, counts.ctypes.data,
            scores.ctypes.data, poses.ctypes.data, C.byref(stats))
    for hole in (0, 1, 3, 4, 5, 6, 7):                 # every pointer but the optional stats
        args = list(good)
        args[hole] = None
        assert host(*args) == _lib.INVALID_ARGUMENT, hole
    for num in (0, -1):
        args = list(good)
        args[2] = num
        assert host(*args) == _lib.INVALID_ARGUMENT, num
    assert host(*good) == _lib.INVALID_ARGUMENT        # a null grid in the list
    good_r = (C.byref(opts), one, 1, poses.ctypes.data, one, scores.ctypes.data,
              poses.ctypes.data, C.byref(stats))
    for hole in (0, 1, 3, 4, 5, 6):
        args = list(good_r)
        args[hole] = None
        assert resident(*args) == _lib.INVALID_ARGUMENT, hole
    assert resident(*good_r) == _lib.INVALID_ARGUMENT  # a null grid and a null cloud in the lists
    assert resident(C.byref(opts), one, 0, poses.ctypes.data, one, scores.ctypes.data,
                    poses.ctypes.data, None) == _lib.INVALID_ARGUMENT


def test_no_cpu_fallback():
    """The issue's case "without a HIP device a valid call returns CMX_DEVICE_ERROR" is NOT
    exercised by this test, and cannot be: a valid call needs cmx_tsdf2d handles, the entries
    read them, and none can exist without a device.  What is checked is the nearest thing that
    can be: creating the grid a batch needs is CMX_DEVICE_ERROR at the C ABI and through the
    Python mirror's grid class, so no path leads to a match computed on the host.  This passes
    on the parent commit too; the test of this file that needs the feature is the symbol test."""
    from cartographer_amd import _lib, grid_2d
    L = _lib.lib()
    if L.cmx_device_count() > 0:
        pytest.skip("a HIP device is present")
    lim = _lib.Grid2DLimits(0.05, 1.0, 1.0, 16, 16, 0.0, 0.0)
    h = C.c_void_p()
    assert L.cmx_tsdf2d_create(C.byref(lim), 0.3, 10.0, None, None, 0, C.byref(h)) == \
        _lib.DEVICE_ERROR
    assert not h
    with pytest.raises(_lib.CmxError) as err:
        grid_2d.TSDF2DOnDevice(0.05, (1.0, 1.0), 16, 16, 0.3, 10.0)
    assert err.value.status == _lib.DEVICE_ERROR
