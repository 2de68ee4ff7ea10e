"""C ABI of the device-resident TSDF2D (CPU): the options struct's layout, no CPU fallback, and the
golden file of tests/test_gpu_tsdf.py regenerating identically wherever oracle/_ref builds."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_tsdf_options_layout_agrees_with_the_header(tmp_path):
    from cartographer_amd import _lib
    header = open(os.path.join(ROOT, "include", "cartographer_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "cmx_tsdf_inserter_options_2d"
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S)
    assert body, name
    fields = [re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", d.strip())[0]
              for d in body.group(1).split(";") if d.strip()]
    mirror = _lib.TSDFInserterOptions2D
    assert fields == [f[0] for f in mirror._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(
        ['#include <stdio.h>', '#include <stddef.h>', '#include "cartographer_mi355x.h"',
         'int main(void) {', f'  printf("%zu", sizeof({name}));'] +
        [f'  printf(" %zu", offsetof({name}, {f}));' for f in fields] +
        ['  printf("\\n");', '  return 0;', '}']))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    words = [int(w) for w in subprocess.run([exe], capture_output=True, text=True,
                                            check=True).stdout.split()]
    assert words[0] == C.sizeof(mirror)
    assert words[1:] == [getattr(mirror, f).offset for f in fields]


def test_no_cpu_fallback_and_argument_checks():
    from cartographer_amd import _lib
    L = _lib.lib()
    if L.cmx_device_count() > 0:
        pytest.skip("a HIP device is present")
    lim = _lib.Grid2DLimits(0.05, 1.0, 1.0, 16, 16, 0.0, 0.0)
    h = C.c_void_p()
    assert L.cmx_tsdf2d_create(C.byref(lim), 0.3, 10.0, None, None, 0, C.byref(h)) == \
        _lib.DEVICE_ERROR
    assert not h
    # argument checks come before the device
    assert L.cmx_tsdf2d_create(C.byref(lim), 0.0, 10.0, None, None, 0, C.byref(h)) == \
        _lib.INVALID_ARGUMENT
    opts = _lib.TSDFInserterOptions2D(0.3, 10.0, 0, 4, 0.5, 1, 0, 0.5, 0.5)
    origin = np.zeros(3, np.float32)
    assert L.cmx_tsdf2d_insert(None, origin.ctypes.data, None, 0, C.byref(opts)) == \
        _lib.INVALID_ARGUMENT
    assert L.cmx_tsdf2d_crop(None) == _lib.INVALID_ARGUMENT
    assert L.cmx_rt2d_match_tsdf_grid(None, None, None, None, 0, None, None, None) == \
        _lib.INVALID_ARGUMENT
    assert L.cmx_fast2d_create_from_tsdf(None, None, C.byref(h)) == _lib.INVALID_ARGUMENT
    L.cmx_tsdf2d_destroy(None)


def test_insert_golden_regenerates_identically(oracle):
    if oracle.ref_lib() is None:
        pytest.skip("reference tree not available and oracle/_ref not prebuilt")
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_tsdf_insert_golden
    fresh = make_tsdf_insert_golden.build()
    stored = np.load(os.path.join(GOLDEN, "tsdf_insert_golden.npz"))
    assert sorted(fresh) == sorted(stored.files)
    for key, value in fresh.items():
        np.testing.assert_array_equal(np.asarray(value), stored[key], err_msg=key)


def test_fast2d_refuses_a_cost_range_with_negative_scores():
    """cmx_fast2d_create checks the range before it touches the device: max_correspondence_cost
    > 1 (a TSDF2D truncated beyond 1 m) would give scores down to 1 - max < 0, which the search
    cannot represent.  CMX_INVALID_ARGUMENT with the reason, with or without a device."""
    from cartographer_amd import _lib
    L = _lib.lib()
    cells = np.zeros((16, 16), np.uint16)
    options = _lib.Fast2DOptions(1.0, 0.3, 3)
    for max_cc in (1.5, float(np.nextafter(np.float32(1.0), np.float32(2.0)))):
        lim = _lib.Grid2DLimits(0.05, 1.0, 1.0, 16, 16, -max_cc, max_cc)
        h = C.c_void_p()
        assert L.cmx_fast2d_create(C.byref(options), C.byref(lim), cells.ctypes.data, 0,
                                   C.byref(h)) == _lib.INVALID_ARGUMENT
        assert not h
        message = L.cmx_last_error().decode()
        assert "max_correspondence_cost" in message and "negative" in message
