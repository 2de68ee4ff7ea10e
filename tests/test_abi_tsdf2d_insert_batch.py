"""CPU-side checks of cmx_tsdf2d_insert_batch (range data into many resident TSDF2D grids in one
call): declared, exported, mirrored with the header's argument count and struct layouts, every
argument check made before the device is touched -- with the index of the failing insertion in
cmx_last_error -- the plan of a call (rounds, the limits a grid has AT every insertion, ray counts,
distinct scans prepared) from the functions the launch path itself asks, against the committed
results of the reference's own inserter (tests/golden/tsdf_insert_golden.npz), and the plain-C++
host preparation as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import make_tsdf_insert_golden as mk  # noqa: E402

NAME = "cmx_tsdf2d_insert_batch"
PLAN = "cmx_debug_tsdf2d_insert_plan"
HEADER = os.path.join(ROOT, "include", "cartographer_mi355x.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "cartographer_mi355x_debug.h")
FIELDS = ["grid", "origin_xyz", "returns_xyz", "num_returns"]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "tsdf_insert_golden.npz")))


def test_header_declares_the_call_and_lists_it():
    text = open(HEADER).read()
    assert NAME in text.split("#ifndef")[0]                       # the entry-point list
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % NAME, stripped, re.S)
    assert m, "not declared"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 3
    assert PLAN in open(DEBUG_HEADER).read()


def test_library_exports_the_call_and_the_mirror_has_its_argument_count():
    from cartographer_amd import _lib
    L = _lib.lib()
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert hasattr(L, NAME), f"{NAME} is not exported"
    assert len(getattr(L, NAME).argtypes) == 3
    assert PLAN in _lib.DEBUG_SYMBOLS
    assert len(getattr(L, PLAN).argtypes) == 9


def _c99_layout(tmp_path, header, struct, fields):
    src = tmp_path / "size.c"
    src.write_text(
        f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\n'
        f'int main(void) {{\n  printf("%zu", sizeof({struct}));\n' +
        "".join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in fields) +
        '  return 0;\n}\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe])
    return [int(w) for w in subprocess.run([exe], capture_output=True, text=True,
                                           check=True).stdout.split()]


def test_insertion_struct_has_the_layout_a_c99_compiler_gives_it(tmp_path):
    """sizeof and member offsets of cmx_tsdf2d_insertion from a C99 program against the ctypes
    mirror; compiling it -pedantic -Werror is also the check that the header is still plain C."""
    from cartographer_amd import _lib
    assert [f[0] for f in _lib.TSDF2DInsertion._fields_] == FIELDS
    words = _c99_layout(tmp_path, "cartographer_mi355x.h", "cmx_tsdf2d_insertion", FIELDS)
    assert words[0] == C.sizeof(_lib.TSDF2DInsertion)
    assert words[1:] == [getattr(_lib.TSDF2DInsertion, f).offset for f in FIELDS]


def test_plan_struct_has_the_layout_a_c99_compiler_gives_it(tmp_path):
    from cartographer_amd import _lib
    fields = [f[0] for f in _lib.DebugTSDF2DInsertion._fields_]
    words = _c99_layout(tmp_path, "cartographer_mi355x_debug.h", "cmx_debug_tsdf2d_insertion",
                        fields)
    assert words[0] == C.sizeof(_lib.DebugTSDF2DInsertion)
    assert words[1:] == [getattr(_lib.DebugTSDF2DInsertion, f).offset for f in fields]


def test_python_mirror_has_the_entry_points():
    import inspect
    from cartographer_amd import grid_2d
    batch = inspect.signature(grid_2d.tsdf_insert_batch).parameters
    assert list(batch) == ["insertions", "options"]
    assert batch["options"].kind is inspect.Parameter.VAR_KEYWORD
    plan = inspect.signature(grid_2d.tsdf_insert_batch_plan).parameters
    assert list(plan) == ["limits", "insertions", "options"]
    assert plan["options"].kind is inspect.Parameter.VAR_KEYWORD
    # the keywords are those of TSDF2DOnDevice.insert
    insert = list(inspect.signature(grid_2d.TSDF2DOnDevice.insert).parameters)[3:]
    assert insert == list(mk.OPTION_KEYS)
    with pytest.raises(TypeError):
        grid_2d.tsdf_insert_batch_plan([], [], **dict(mk.LUA_DEFAULTS, no_such_option=1))


def test_debug_switch_exists():
    from cartographer_amd import _lib
    try:
        _lib.debug_set(tsdf2d_insert_chain=2)
    finally:
        _lib.debug_reset()


# ---- argument checks ------------------------------------------------------------------------
def _options(**changes):
    from cartographer_amd import grid_2d
    return grid_2d._tsdf_options(**dict(mk.LUA_DEFAULTS, **changes))


class _Call:
    """Four insertions whose grids are stand-ins (zeroed memory, never a real handle): every check
    these tests reach is made before a grid is looked into."""

    def __init__(self, num=4):
        from cartographer_amd import _lib
        self.lib = _lib
        self.num = num
        self.stand_ins = [C.create_string_buffer(4096) for _ in range(num)]
        self.origin = np.zeros(3, np.float32)
        self.points = np.ones((3, 3), np.float32)
        self.options = _options()
        self.items = (_lib.TSDF2DInsertion * num)()
        for k, item in enumerate(self.items):
            item.grid = C.addressof(self.stand_ins[k])
            item.origin_xyz = self.origin.ctypes.data
            item.returns_xyz, item.num_returns = self.points.ctypes.data, 3

    def __call__(self, items="own", num=None, options="own"):
        return self.lib.lib().cmx_tsdf2d_insert_batch(
            self.items if items == "own" else items, self.num if num is None else num,
            C.byref(self.options) if options == "own" else options)

    def error(self):
        return self.lib.lib().cmx_last_error().decode()


def test_null_insertions_and_empty_lists_are_invalid():
    call = _Call()
    assert call(items=None) == call.lib.INVALID_ARGUMENT
    assert call(num=0) == call.lib.INVALID_ARGUMENT
    assert "num_insertions" in call.error()
    assert call(num=-3) == call.lib.INVALID_ARGUMENT


def test_a_null_grid_in_third_place_is_named():
    call = _Call()
    call.items[2].grid = None
    assert call() == call.lib.INVALID_ARGUMENT
    assert "insertion 2" in call.error(), call.error()


def test_a_null_origin_and_bad_range_data_are_named():
    call = _Call()
    call.items[1].origin_xyz = None
    assert call() == call.lib.INVALID_ARGUMENT
    assert "insertion 1" in call.error(), call.error()
    call = _Call()
    call.items[2].num_returns = -1
    assert call() == call.lib.INVALID_ARGUMENT
    assert "insertion 2" in call.error(), call.error()
    call = _Call()
    call.items[3].returns_xyz, call.items[3].num_returns = None, 2
    assert call() == call.lib.INVALID_ARGUMENT
    assert "insertion 3" in call.error(), call.error()


def test_null_and_bad_options_are_invalid():
    call = _Call()
    assert call(options=None) == call.lib.INVALID_ARGUMENT
    assert "options" in call.error()
    call.options = _options(num_normal_samples=0)
    assert call() == call.lib.INVALID_ARGUMENT
    assert "num_normal_samples" in call.error()
    call.options = _options(sample_radius=0.0)
    assert call() == call.lib.INVALID_ARGUMENT
    assert "sample_radius" in call.error()


# ---- the plan -------------------------------------------------------------------------------
def _limits_of(meta):
    res, mx, my, nx, ny = meta[:5]
    return dict(resolution=float(res), max_x=float(mx), max_y=float(my), num_x_cells=int(nx),
                num_y_cells=int(ny))


def _limits_array(lim):
    return np.array([lim["resolution"], lim["max_x"], lim["max_y"], lim["num_x_cells"],
                     lim["num_y_cells"]], np.float64)


def _ranges(origin, returns):
    d = np.asarray(returns, np.float32)[:, :2] - np.asarray(origin, np.float32)[:2]
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def test_plan_of_the_room_scans_has_the_limits_of_the_reference_at_every_insertion(golden):
    """(a) twelve scans, twelve rounds on one 16 x 16 grid that grows on the way."""
    from cartographer_amd import grid_2d
    steps = [mk.step_inputs(golden, "room_lua", k) for k in range(12)]
    insertions = [(0, origin, returns) for origin, returns, _, _ in steps]
    rounds, at, rays, scans = grid_2d.tsdf_insert_batch_plan(
        [_limits_of(golden["room_lua/meta"])], insertions, **mk.LUA_DEFAULTS)
    assert rounds == list(range(12))
    assert scans == 12
    for k in range(12):
        np.testing.assert_array_equal(_limits_array(at[k]), golden[f"room_lua/{k}/limits"],
                                      err_msg=f"insertion {k}")
    assert at[0]["num_x_cells"] > 16                               # the first scan grows it
    # No hit is closer than 0.47 m (to the centimetre: the nearest of all is at 0.4694 m), well
    # clear of the truncation distance of 0.3 m: every return is a ray.
    nearest = min(float(_ranges(origin, returns).min()) for origin, returns, _, _ in steps)
    assert round(nearest, 2) >= 0.47 and nearest > 0.3 + 0.16
    for (origin, returns, _, _), n in zip(steps, rays):
        assert n == returns.shape[0]


def test_plan_counts_rays_not_returns_and_grows_for_an_empty_insertion(golden):
    """(b) `edges` steps 2 (every third hit at 0.15 m, inside the truncation distance) and 4 (no
    returns, an origin outside the grid)."""
    from cartographer_amd import grid_2d
    o2, r2, opts2, _ = mk.step_inputs(golden, "edges", 2)
    o4, r4, opts4, _ = mk.step_inputs(golden, "edges", 4)
    assert opts2 == mk.LUA_DEFAULTS and opts4 == mk.LUA_DEFAULTS
    near = _ranges(o2, r2) < 0.3
    assert r2.shape[0] == 120 and near.sum() == 40 and r4.shape[0] == 0
    np.testing.assert_allclose(_ranges(o2, r2)[near], 0.15, atol=1e-6)
    rounds, at, rays, scans = grid_2d.tsdf_insert_batch_plan(
        [_limits_of(golden["edges/meta"])], [(0, o2, r2), (0, o4, r4)], **mk.LUA_DEFAULTS)
    assert rounds == [0, 1] and rays == [80, 0] and scans == 1
    assert (at[0]["num_x_cells"], at[0]["num_y_cells"]) == (128, 128)
    assert (at[1]["num_x_cells"], at[1]["num_y_cells"]) == (256, 256)
    np.testing.assert_array_equal(golden["edges/3/limits"][3:], [128, 128])
    np.testing.assert_array_equal(_limits_array(at[1]), golden["edges/4/limits"])


def test_plan_prepares_every_distinct_scan_once(golden):
    """(c) three grids, every scan into two of them by the same array object."""
    from cartographer_amd import grid_2d
    limits = [_limits_of(golden["room_lua/meta"])] * 3
    insertions = []
    for k in range(5):
        origin, returns, _, _ = mk.step_inputs(golden, "room_lua", k)
        insertions += [(k % 3, origin, returns), ((k + 1) % 3, origin, returns)]
    rounds, at, rays, scans = grid_2d.tsdf_insert_batch_plan(limits, insertions,
                                                             **mk.LUA_DEFAULTS)
    assert scans == 5 and len(rays) == 10
    assert rays[0::2] == rays[1::2]
    assert max(rounds) == 3                    # ten insertions over three grids: 4 + 3 + 3
    # the same pointer from another origin is another scan
    origin, returns, _, _ = mk.step_inputs(golden, "room_lua", 0)
    moved = origin + np.array([0.01, 0.0, 0.0], np.float32)
    assert grid_2d.tsdf_insert_batch_plan(limits, [(0, origin, returns), (1, moved, returns)],
                                          **mk.LUA_DEFAULTS)[3] == 2


def _ring(radius):
    a = 2.0 * np.pi * (np.arange(64) + 0.25) / 64
    return np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(64)], 1).astype(np.float32)


RING_GRID = dict(resolution=0.05, max_x=0.4, max_y=0.4, num_x_cells=16, num_y_cells=16)


def test_plan_gives_an_insertion_the_limits_of_its_own_moment():
    """(d) rings of 1.0, 1.1, 2.5 and 1.2 m into a 16 x 16 grid at 5 cm centred on the origin: with
    the truncation distance of 0.3 m the ray ends reach 1.3, 1.4, 2.8 and 1.5 m; doubling keeps the
    centre, so the grid spans +-0.4, 0.8, 1.6, 3.2 m at 16, 32, 64, 128 cells."""
    from cartographer_amd import grid_2d
    insertions = [(0, (0.0, 0.0, 0.0), _ring(r)) for r in (1.0, 1.1, 2.5, 1.2)]
    rounds, at, rays, scans = grid_2d.tsdf_insert_batch_plan([RING_GRID], insertions,
                                                             **mk.LUA_DEFAULTS)
    assert rounds == [0, 1, 2, 3] and rays == [64] * 4 and scans == 4
    assert [l["num_x_cells"] for l in at] == [64, 64, 128, 128]
    assert [l["num_y_cells"] for l in at] == [64, 64, 128, 128]
    assert [(l["max_x"], l["max_y"]) for l in at] == [(1.6, 1.6)] * 2 + [(3.2, 3.2)] * 2


def test_plan_names_the_insertion_whose_range_data_leaves_the_limits():
    """(e) z != 0 shortens the box GrowAsNeeded builds from 3D directions: the 2D ray end lies
    outside the grown grid."""
    from cartographer_amd import _lib, grid_2d
    limits = [dict(resolution=0.05, max_x=1.0, max_y=1.0, num_x_cells=16, num_y_cells=16)]
    fine = np.array([[0.5, 0.5, 0.0]], np.float32)
    far = np.array([[3.5, 0.0, 30.0]], np.float32)
    opts = dict(mk.LUA_DEFAULTS, truncation_distance=0.5)
    with pytest.raises(_lib.CmxError) as e:
        grid_2d.tsdf_insert_batch_plan(limits, [(0, (0, 0, 0), fine), (0, (0, 0, 0), far),
                                                (0, (0, 0, 0), fine)], **opts)
    assert e.value.status == _lib.INVALID_ARGUMENT and "insertion 1" in str(e.value)
    grid_2d.tsdf_insert_batch_plan(limits, [(0, (0, 0, 0), fine)] * 3, **opts)


def test_plan_refuses_one_pointer_with_two_counts():
    """(f)"""
    from cartographer_amd import _lib
    L = _lib.lib()
    limits = _lib.Grid2DLimits(0.05, 0.4, 0.4, 16, 16, 0.0, 0.0)
    origin = np.zeros(3, np.float32)
    points = _ring(1.0)
    items = (_lib.DebugTSDF2DInsertion * 3)()
    for item, n in zip(items, (64, 64, 63)):
        item.grid, item.num_returns = 0, n
        item.origin_xyz, item.returns_xyz = origin.ctypes.data, points.ctypes.data
    rounds, rays = np.zeros(3, np.int32), np.zeros(3, np.int32)
    at = (_lib.Grid2DLimits * 3)()
    scans = C.c_int32()
    options = _options()
    status = L.cmx_debug_tsdf2d_insert_plan(C.byref(limits), 1, items, 3, C.byref(options),
                                            rounds.ctypes.data, at, rays.ctypes.data,
                                            C.byref(scans))
    assert status == _lib.INVALID_ARGUMENT
    assert "insertion 2" in L.cmx_last_error().decode()
    assert "64" in L.cmx_last_error().decode() and "63" in L.cmx_last_error().decode()


def test_plan_refuses_a_grid_that_would_pass_2_30_cells():
    from cartographer_amd import _lib, grid_2d
    limits = [dict(resolution=0.001, max_x=8.0, max_y=8.0, num_x_cells=16384, num_y_cells=16384)]
    far = np.array([[1e6, 0.0, 0.0]], np.float32)
    with pytest.raises(_lib.CmxError) as e:
        grid_2d.tsdf_insert_batch_plan(limits, [(0, (0.0, 0.0, 0.0), None),
                                                (0, (0.0, 0.0, 0.0), far)], **mk.LUA_DEFAULTS)
    assert e.value.status == _lib.INVALID_ARGUMENT and "insertion 1" in str(e.value)


# ---- the host preparation alone --------------------------------------------------------------
def test_host_preparation_is_the_same_serially_and_over_threads_under_sanitizers(tmp_path):
    exe = tmp_path / "tsdf2d_prepare_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cartographer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "tsdf2d_prepare_check.cc"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "rays 512 failures 0" in out.stdout
