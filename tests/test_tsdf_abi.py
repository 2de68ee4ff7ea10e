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
