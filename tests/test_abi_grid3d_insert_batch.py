"""CPU-side checks of cmx_grid3d_insert_batch (range data into many resident hybrid grids in one
call): declared, exported, mirrored with the header's argument count and struct layout, every
argument check made before the device is touched -- with the index of the failing insertion in
cmx_last_error -- and the plan of a call (the round of every insertion, the brick bounds and
grid_size of every grid afterwards) from the function the launch path itself asks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cmx_grid3d_insert_batch"
PLAN = "cmx_debug_grid3d_insert_plan"
HEADER = os.path.join(ROOT, "include", "cartographer_mi355x.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "cartographer_mi355x_debug.h")
FIELDS = ["grid", "origin_xyz", "returns_xyz", "num_returns", "reserved"]


def test_header_declares_the_call_and_lists_it():
    text = open(HEADER).read()
    assert NAME in text.split("#ifndef")[0]                       # the entry-point list
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % NAME, stripped, re.S)
    assert m, "not declared"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 5
    assert stripped.index("cmx_grid3d_insert(") < m.start() < stripped.index("cmx_grid3d_info(")
    assert PLAN in open(DEBUG_HEADER).read()


def test_library_exports_the_call_and_the_mirror_has_its_argument_count():
    from cartographer_amd import _lib
    L = _lib.lib()
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert hasattr(L, NAME), f"{NAME} is not exported"
    assert len(getattr(L, NAME).argtypes) == 5
    assert PLAN in _lib.DEBUG_SYMBOLS
    assert len(getattr(L, PLAN).argtypes) == 6


def _layout(tmp_path, header, struct, fields):
    """sizeof and member offsets of `struct` from a C99 program; compiling it -pedantic -Werror is
    also the check that the header is still plain C."""
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
    from cartographer_amd import _lib
    assert [f[0] for f in _lib.Grid3DInsertion._fields_] == FIELDS
    words = _layout(tmp_path, "cartographer_mi355x.h", "cmx_grid3d_insertion", FIELDS)
    assert words[0] == C.sizeof(_lib.Grid3DInsertion)
    assert words[1:] == [getattr(_lib.Grid3DInsertion, f).offset for f in FIELDS]


@pytest.mark.parametrize("struct,mirror", [("cmx_debug_grid3d_state", "DebugGrid3DState"),
                                           ("cmx_debug_grid3d_insertion", "DebugGrid3DInsertion")])
def test_plan_structs_have_the_layout_a_c99_compiler_gives_them(tmp_path, struct, mirror):
    from cartographer_amd import _lib
    mirror = getattr(_lib, mirror)
    fields = [f[0] for f in mirror._fields_]
    words = _layout(tmp_path, "cartographer_mi355x_debug.h", struct, fields)
    assert words[0] == C.sizeof(mirror)
    assert words[1:] == [getattr(mirror, f).offset for f in fields]


def test_python_mirror_has_the_entry_points():
    import inspect
    from cartographer_amd import grid_3d
    parameters = inspect.signature(grid_3d.insert_batch).parameters
    assert list(parameters) == ["insertions", "hit_probability", "miss_probability",
                                "num_free_space_voxels"]
    assert parameters["hit_probability"].default == 0.7
    assert parameters["miss_probability"].default == 0.4
    assert parameters["num_free_space_voxels"].default == 5
    assert list(inspect.signature(grid_3d.insert_batch_plan).parameters) == ["grids", "insertions"]


def test_debug_switch_exists():
    from cartographer_amd import _lib
    try:
        _lib.debug_set(grid3d_insert_chain=2)
    finally:
        _lib.debug_reset()


# ---- argument checks ------------------------------------------------------------------------
class _Call:
    """Four insertions whose grids are stand-ins (zeroed memory, never a real handle): every check
    these tests reach is made before the device is touched.  The one member a check reads from a
    grid is its device, the int the handle begins with."""

    def __init__(self, num=4):
        from cartographer_amd import _lib
        self.lib = _lib
        self.num = num
        self.stand_ins = [C.create_string_buffer(4096) for _ in range(num)]
        self.origin = np.zeros(3, np.float32)
        self.points = np.ones((3, 3), np.float32)
        self.items = (_lib.Grid3DInsertion * num)()
        for k, item in enumerate(self.items):
            item.grid = C.addressof(self.stand_ins[k])
            item.origin_xyz = self.origin.ctypes.data
            item.returns_xyz, item.num_returns = self.points.ctypes.data, 3

    def __call__(self, items="own", num=None, hit=0.55, miss=0.49, free=2):
        return self.lib.lib().cmx_grid3d_insert_batch(
            self.items if items == "own" else items, self.num if num is None else num, hit, miss,
            free)

    def error(self):
        return self.lib.lib().cmx_last_error().decode()


def test_null_insertions_and_empty_lists_are_invalid():
    call = _Call()
    assert call(items=None) == call.lib.INVALID_ARGUMENT
    assert call(num=0) == call.lib.INVALID_ARGUMENT
    assert "num_insertions" in call.error()
    assert call(num=-3) == call.lib.INVALID_ARGUMENT


def test_call_wide_arguments_are_checked():
    call = _Call()
    assert call(free=-1) == call.lib.INVALID_ARGUMENT
    assert "num_free_space_voxels" in call.error()
    for hit, miss in [(0.0, 0.4), (1.0, 0.4), (0.7, 0.0), (0.7, 1.0), (-0.1, 0.4), (0.7, 1.5),
                      (float("nan"), 0.4)]:
        assert call(hit=hit, miss=miss) == call.lib.INVALID_ARGUMENT, (hit, miss)
        assert "probability" in call.error()


@pytest.mark.parametrize("index", [0, 2, 3])
def test_every_rule_names_the_insertion_first_middle_and_last(index):
    def broken(change):
        call = _Call()
        change(call.items[index], call)
        assert call() == call.lib.INVALID_ARGUMENT
        assert f"insertion {index}" in call.error(), call.error()

    broken(lambda item, call: setattr(item, "grid", None))
    broken(lambda item, call: setattr(item, "origin_xyz", None))
    broken(lambda item, call: setattr(item, "num_returns", -1))
    broken(lambda item, call: setattr(item, "returns_xyz", None))   # num_returns is 3
    broken(lambda item, call: setattr(item, "reserved", 1))


@pytest.mark.parametrize("index", [1, 3])
def test_grids_on_different_devices_are_named(index):
    call = _Call()
    C.c_int32.from_buffer(call.stand_ins[index]).value = 1          # the handle's `device`
    assert call() == call.lib.INVALID_ARGUMENT
    assert f"insertion {index}" in call.error() and "device" in call.error(), call.error()


def test_one_pointer_with_two_counts_is_named():
    call = _Call()
    call.items[2].num_returns = 2
    assert call() == call.lib.INVALID_ARGUMENT
    assert "insertion 2" in call.error(), call.error()


# ---- the plan -------------------------------------------------------------------------------
EMPTY = dict(lo=None, dims=None, grid_size=128)


def _plan(grids, insertions):
    from cartographer_amd import grid_3d
    return grid_3d.insert_batch_plan(grids, insertions)


def _replay(grids, insertions):
    """The growth steps of the single call, restated: per insertion the brick becomes the union
    with the box floored / ceiled to multiples of 16, grid_size doubles until the box fits."""
    state = [dict(g) for g in grids]
    for g, box in insertions:
        if box is None:
            continue
        s = state[g]
        lo = [v // 16 * 16 for v in box[:3]]
        hi = [v // 16 * 16 + 15 for v in box[3:]]
        if s["dims"] is not None:
            lo = [min(a, b) for a, b in zip(lo, s["lo"])]
            hi = [max(a, b + d - 1) for a, b, d in zip(hi, s["lo"], s["dims"])]
        s["lo"], s["dims"] = tuple(lo), tuple(h - l + 1 for l, h in zip(lo, hi))
        while not all(-(s["grid_size"] // 2) <= v < s["grid_size"] // 2 for v in box):
            s["grid_size"] *= 2
    return state


def test_plan_gives_the_rounds_of_an_interleaved_list_and_the_union_of_the_aligned_boxes():
    """Three grids with 3, 1 and 2 insertions; grid 0 starts with a brick, negative coordinates
    on every axis (FloorTo rounds towards minus infinity)."""
    grids = [dict(lo=(-16, 0, -32), dims=(32, 16, 48), grid_size=128), dict(EMPTY), dict(EMPTY)]
    insertions = [(0, (-17, 3, -1, 5, 9, 2)), (1, (-1, -16, -33, 0, -1, -17)),
                  (2, (1, 1, 1, 1, 1, 1)), (0, (0, 0, 0, 31, 40, 3)), (2, (-40, 15, 16, -3, 16, 31)),
                  (0, (-5, -5, -5, -4, -4, -4))]
    rounds, final = _plan(grids, insertions)
    assert rounds == [0, 0, 0, 1, 1, 2]
    assert final == _replay(grids, insertions)
    assert final[0] == dict(lo=(-32, -16, -32), dims=(64, 64, 48), grid_size=128)
    assert final[1] == dict(lo=(-16, -16, -48), dims=(32, 16, 32), grid_size=128)
    assert final[2] == dict(lo=(-48, 0, 0), dims=(64, 32, 32), grid_size=128)


def test_plan_doubles_grid_size_at_the_edge_of_64_voxels():
    """Index 64 fits nowhere in a grid of 128 (its indices are -64 .. 63); -64 does."""
    _, final = _plan([dict(EMPTY), dict(EMPTY), dict(EMPTY)],
                     [(0, (-64, -64, -64, 63, 63, 63)), (1, (0, 0, 0, 0, 64, 0)),
                      (2, (0, 0, -65, 0, 0, 0)), (2, (0, 0, 0, 300, 0, 0))])
    assert [f["grid_size"] for f in final] == [128, 256, 1024]
    assert final[0]["lo"] == (-64, -64, -64) and final[0]["dims"] == (128, 128, 128)
    assert final[1]["lo"] == (0, 0, 0) and final[1]["dims"] == (16, 80, 16)


def test_plan_leaves_a_grid_alone_whose_insertions_touch_nothing():
    """An insertion without returns has no box: it takes its round and changes nothing, on an
    empty grid and on one with a brick."""
    with_brick = dict(lo=(0, 0, 0), dims=(16, 16, 16), grid_size=256)
    rounds, final = _plan([dict(EMPTY), with_brick],
                          [(0, None), (1, None), (1, (1, 2, 3, 4, 5, 6)), (0, None), (1, None)])
    assert rounds == [0, 0, 1, 1, 2]
    assert final == [EMPTY, with_brick]


@pytest.mark.parametrize("box", [(0, 0, 0, 2**20, 0, 0), (0, -2**20, 0, 0, 0, 0),
                                 (0, 0, -2**20 - 5, 0, 0, 0)])
def test_plan_refuses_a_voxel_index_at_2_20(box):
    from cartographer_amd import _lib
    with pytest.raises(_lib.CmxError) as e:
        _plan([dict(EMPTY), dict(EMPTY)], [(0, (0, 0, 0, 1, 1, 1)), (1, box)])
    assert e.value.status == _lib.INVALID_ARGUMENT and "insertion 1" in str(e.value)
    # one voxel inside the bound is planned
    _, final = _plan([dict(EMPTY)], [(0, (-2**20 + 1, 0, 0, -2**20 + 1, 0, 0))])
    assert final[0]["lo"][0] == -2**20 and final[0]["grid_size"] == 2**21
