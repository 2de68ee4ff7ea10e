"""C ABI of Ceres refinement on a TSDF2D (CPU): the header declares what the library exports, a
C99 program calling the four entry points links, argument checks come before the device, no
CPU fallback, and the golden file of tests/test_gpu_ceres_tsdf.py regenerates identically
wherever the reference builds."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRY_POINTS = ["cmx_ceres2d_match_tsdf", "cmx_ceres2d_match_tsdf_grid",
                "cmx_ceres2d_refine_batch_tsdf", "cmx_ceres2d_tsdf_residuals"]


def test_header_and_exported_symbols_agree():
    from cartographer_amd import _lib
    header = open(os.path.join(ROOT, "include", "cartographer_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"cmx_status\s+%s\(" % name, code), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert name in header.split("#ifndef")[0], name        # the entry-point list
        assert hasattr(_lib.lib(), name)


def test_header_compiles_as_c99_and_links(tmp_path):
    from cartographer_amd import _lib
    src = tmp_path / "tsdf_ceres.c"
    src.write_text("""#include <stdio.h>
#include "cartographer_mi355x.h"
int main(void) {
  cmx_ceres2d_options o = {1.0, 10.0, 40.0, 0, 20};
  cmx_grid2d_limits lim = {0.05, 1.0, 1.0, 4, 4, 0.f, 0.f};
  uint16_t tsd[16] = {0}, weight[16] = {0};
  double target[2] = {0.0, 0.0}, pose3[3] = {0.0, 0.0, 0.0}, r[1], J[3];
  float xyz[3] = {0.f, 0.f, 0.f};
  cmx_pose2d init = {0.0, 0.0, 0.0}, out;
  cmx_ceres_summary s;
  int32_t valid = 0, found = 1;
  const cmx_tsdf2d* grids[1] = {NULL};
  cmx_status a = cmx_ceres2d_match_tsdf(&o, &lim, tsd, weight, 0.3f, 10.f, target, &init, xyz, 1,
                                        0, &out, &s);
  cmx_status b = cmx_ceres2d_match_tsdf_grid(&o, NULL, target, &init, xyz, 1, &out, &s);
  cmx_status c = cmx_ceres2d_refine_batch_tsdf(&o, grids, 1, &found, &init, xyz, 1, &out, &s);
  cmx_status d = cmx_ceres2d_tsdf_residuals(&lim, tsd, weight, 0.3f, 10.f, 1.0, pose3, xyz, 1, 0,
                                            r, J, &valid);
  printf("%d %d %d %d\\n", (int)a, (int)b, (int)c, (int)d);
  return 0;
}
""")
    exe = str(tmp_path / "tsdf_ceres")
    lib_dir = os.path.dirname(_lib.SO_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L", lib_dir, "-lcartographer_mi355x",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    status = [int(w) for w in out.stdout.split()]
    assert status[1] == 1 and status[2] == 1                     # null grids: INVALID_ARGUMENT
    if _lib.lib().cmx_device_count() == 0:
        assert status[0] == 2 and status[3] == 2                 # CMX_DEVICE_ERROR


def _args():
    from cartographer_amd import _lib
    o = _lib.Ceres2DOptions(1.0, 10.0, 40.0, 0, 20)
    lim = _lib.Grid2DLimits(0.05, 1.0, 1.0, 8, 8, 0.0, 0.0)
    planes = np.zeros((8, 8), np.uint16), np.zeros((8, 8), np.uint16)
    return o, lim, planes


def test_argument_checks_come_before_the_device():
    from cartographer_amd import _lib
    L = _lib.lib()
    o, lim, (tsd, wgt) = _args()
    target = np.zeros(2)
    xyz = np.zeros((4, 3), np.float32)
    init, pose, s = _lib.Pose2d(), _lib.Pose2d(), _lib.CeresSummary()
    bad = _lib.INVALID_ARGUMENT

    def match(**kw):
        a = dict(o=C.byref(o), lim=C.byref(lim), tsd=tsd.ctypes.data, wgt=wgt.ctypes.data,
                 trunc=0.3, maxw=10.0, target=target.ctypes.data, init=C.byref(init),
                 xyz=xyz.ctypes.data, n=4, dev=0, pose=C.byref(pose), s=C.byref(s))
        a.update(kw)
        return L.cmx_ceres2d_match_tsdf(*a.values())

    assert match(o=None) == bad
    assert match(lim=None) == bad
    assert match(tsd=None) == bad
    assert match(wgt=None) == bad
    assert match(trunc=0.0) == bad
    assert match(maxw=-1.0) == bad
    assert match(target=None) == bad
    assert match(init=None) == bad
    assert match(pose=None) == bad
    assert match(n=-1) == bad
    assert match(xyz=None) == bad                              # n > 0 needs a cloud
    bad_opts = _lib.Ceres2DOptions(0.0, 10.0, 40.0, 0, 20)
    assert match(o=C.byref(bad_opts)) == bad
    bad_lim = _lib.Grid2DLimits(0.0, 1.0, 1.0, 8, 8, 0.0, 0.0)
    assert match(lim=C.byref(bad_lim)) == bad

    assert L.cmx_ceres2d_match_tsdf_grid(C.byref(o), None, target.ctypes.data, C.byref(init),
                                         xyz.ctypes.data, 4, C.byref(pose), C.byref(s)) == bad
    handles = (C.c_void_p * 1)(None)
    assert L.cmx_ceres2d_refine_batch_tsdf(C.byref(o), handles, 1, None, C.byref(init),
                                           xyz.ctypes.data, 4, C.byref(pose), C.byref(s)) == bad
    assert L.cmx_ceres2d_refine_batch_tsdf(C.byref(o), None, 1, None, C.byref(init),
                                           xyz.ctypes.data, 4, C.byref(pose), C.byref(s)) == bad
    assert L.cmx_ceres2d_refine_batch_tsdf(C.byref(o), handles, 0, None, C.byref(init),
                                           xyz.ctypes.data, 4, C.byref(pose), C.byref(s)) == bad

    p3 = np.zeros(3)
    r, J = np.zeros(4), np.zeros(12)
    valid = C.c_int32()

    def residuals(**kw):
        a = dict(lim=C.byref(lim), tsd=tsd.ctypes.data, wgt=wgt.ctypes.data, trunc=0.3,
                 maxw=10.0, scaling=1.0, pose=p3.ctypes.data, xyz=xyz.ctypes.data, n=4, dev=0,
                 r=r.ctypes.data, J=J.ctypes.data, valid=C.byref(valid))
        a.update(kw)
        return L.cmx_ceres2d_tsdf_residuals(*a.values())

    for key in ("lim", "tsd", "wgt", "pose", "xyz", "r", "J", "valid"):
        assert residuals(**{key: None}) == bad, key
    assert residuals(n=-2) == bad
    assert residuals(trunc=-0.3) == bad


def test_no_cpu_fallback():
    from cartographer_amd import _lib
    L = _lib.lib()
    if L.cmx_device_count() > 0:
        pytest.skip("a HIP device is present")
    o, lim, (tsd, wgt) = _args()
    target = np.zeros(2)
    xyz = np.zeros((4, 3), np.float32)
    init, pose, s = _lib.Pose2d(), _lib.Pose2d(), _lib.CeresSummary()
    assert L.cmx_ceres2d_match_tsdf(C.byref(o), C.byref(lim), tsd.ctypes.data, wgt.ctypes.data,
                                    0.3, 10.0, target.ctypes.data, C.byref(init),
                                    xyz.ctypes.data, 4, 0, C.byref(pose), C.byref(s)) == \
        _lib.DEVICE_ERROR
    # an empty cloud is a valid request (the reference's solve then fails): it reaches the device
    assert L.cmx_ceres2d_match_tsdf(C.byref(o), C.byref(lim), tsd.ctypes.data, wgt.ctypes.data,
                                    0.3, 10.0, target.ctypes.data, C.byref(init), None, 0, 0,
                                    C.byref(pose), C.byref(s)) == _lib.DEVICE_ERROR
    valid = C.c_int32()
    assert L.cmx_ceres2d_tsdf_residuals(C.byref(lim), tsd.ctypes.data, wgt.ctypes.data, 0.3, 10.0,
                                        1.0, np.zeros(3).ctypes.data, xyz.ctypes.data, 4, 0,
                                        np.zeros(4).ctypes.data, np.zeros(12).ctypes.data,
                                        C.byref(valid)) == _lib.DEVICE_ERROR
    from cartographer_amd import scan_matching as sm
    grid = sm.TSDF2D(tsd, wgt, 0.05, 1.0, 1.0, 0.3, 10.0)
    with pytest.raises(_lib.CmxError) as err:
        sm.CeresScanMatcher2D(1.0, 10.0, 40.0).match([0, 0], sm.Rigid2d(), xyz, grid)
    assert err.value.status == _lib.DEVICE_ERROR


def test_golden_regenerates_identically(oracle):
    if not os.path.isdir("/root/reference") and oracle.ref_ceres_lib() is None:
        pytest.skip("reference tree not available and oracle/_ref not prebuilt")
    if not os.path.isdir("/root/reference"):
        pytest.skip("the driver compiles against the reference's headers")
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_ceres2d_tsdf_golden
    fresh = make_ceres2d_tsdf_golden.build()
    stored = np.load(os.path.join(GOLDEN, "ceres2d_tsdf_golden.npz"))
    assert sorted(fresh) == sorted(stored.files)
    for key, value in fresh.items():
        np.testing.assert_array_equal(np.asarray(value), stored[key], err_msg=key)
