"""CPU-side checks of cmx_grid2d_insert_batch (range data into many resident probability grids in
one call): declared, exported, mirrored with the header's argument count and struct layout, every
argument check made before the device is touched -- with the index of the failing insertion in
cmx_last_error -- and the plan of a call (the round of every insertion, the limits of every grid
afterwards) from the function the launch path itself asks, against the host restatement of the
inserter that tests/test_reference_ref_grid.py pins to the reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cmx_grid2d_insert_batch"
HEADER = os.path.join(ROOT, "include", "cartographer_mi355x.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "cartographer_mi355x_debug.h")
FIELDS = ["grid", "origin_xy", "returns_xyz", "num_returns", "misses_xyz", "num_misses"]


def test_header_declares_the_call_and_lists_it():
    text = open(HEADER).read()
    assert NAME in text.split("#ifndef")[0]                       # the entry-point list
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % NAME, stripped, re.S)
    assert m, "not declared"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 5
    assert "cmx_debug_grid2d_insert_plan" in open(DEBUG_HEADER).read()


def test_library_exports_the_call_and_the_mirror_has_its_argument_count():
    from cartographer_amd import _lib
    L = _lib.lib()
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert hasattr(L, NAME), f"{NAME} is not exported"
    assert len(getattr(L, NAME).argtypes) == 5
    assert "cmx_debug_grid2d_insert_plan" in _lib.DEBUG_SYMBOLS
    assert len(L.cmx_debug_grid2d_insert_plan.argtypes) == 6


def test_insertion_struct_has_the_layout_a_c99_compiler_gives_it(tmp_path):
    """sizeof and member offsets of cmx_grid2d_insertion from a C99 program against the ctypes
    mirror; compiling it -pedantic -Werror is also the check that the header is still plain C."""
    from cartographer_amd import _lib
    assert [f[0] for f in _lib.Grid2DInsertion._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cartographer_mi355x.h"\n'
        'int main(void) {\n  printf("%zu", sizeof(cmx_grid2d_insertion));\n' +
        "".join(f'  printf(" %zu", offsetof(cmx_grid2d_insertion, {f}));\n' for f in FIELDS) +
        '  return 0;\n}\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe])
    words = [int(w) for w in subprocess.run([exe], capture_output=True, text=True,
                                            check=True).stdout.split()]
    assert words[0] == C.sizeof(_lib.Grid2DInsertion)
    assert words[1:] == [getattr(_lib.Grid2DInsertion, f).offset for f in FIELDS]


def test_plan_struct_has_the_layout_a_c99_compiler_gives_it(tmp_path):
    from cartographer_amd import _lib
    fields = [f[0] for f in _lib.DebugGrid2DInsertion._fields_]
    src = tmp_path / "size.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cartographer_mi355x_debug.h"\n'
        'int main(void) {\n  printf("%zu", sizeof(cmx_debug_grid2d_insertion));\n' +
        "".join(f'  printf(" %zu", offsetof(cmx_debug_grid2d_insertion, {f}));\n'
                for f in fields) +
        '  return 0;\n}\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe])
    words = [int(w) for w in subprocess.run([exe], capture_output=True, text=True,
                                            check=True).stdout.split()]
    assert words[0] == C.sizeof(_lib.DebugGrid2DInsertion)
    assert words[1:] == [getattr(_lib.DebugGrid2DInsertion, f).offset for f in fields]


def test_python_mirror_has_the_entry_points():
    import inspect
    from cartographer_amd import grid_2d
    parameters = inspect.signature(grid_2d.insert_batch).parameters
    assert list(parameters) == ["insertions", "hit_probability", "miss_probability",
                                "insert_free_space"]
    assert parameters["hit_probability"].default == 0.7
    assert parameters["miss_probability"].default == 0.4
    assert parameters["insert_free_space"].default is True
    assert list(inspect.signature(grid_2d.insert_batch_plan).parameters) == ["limits",
                                                                             "insertions"]


def test_debug_switch_exists():
    from cartographer_amd import _lib
    try:
        _lib.debug_set(grid2d_insert_chain=2)
    finally:
        _lib.debug_reset()


# ---- argument checks ------------------------------------------------------------------------
class _Call:
    """Four insertions whose grids are stand-ins (zeroed memory, never a real handle): every check
    these tests reach is made before a grid is looked into."""

    def __init__(self, num=4):
        from cartographer_amd import _lib
        self.lib = _lib
        self.num = num
        self.stand_ins = [C.create_string_buffer(4096) for _ in range(num)]
        self.origin = np.zeros(2, np.float32)
        self.points = np.ones((3, 3), np.float32)
        self.items = (_lib.Grid2DInsertion * num)()
        for k, item in enumerate(self.items):
            item.grid = C.addressof(self.stand_ins[k])
            item.origin_xy = self.origin.ctypes.data
            item.returns_xyz, item.num_returns = self.points.ctypes.data, 3
            item.misses_xyz, item.num_misses = None, 0

    def __call__(self, items="own", num=None, hit=0.55, miss=0.49):
        return self.lib.lib().cmx_grid2d_insert_batch(
            self.items if items == "own" else items, self.num if num is None else num, hit, miss,
            1)

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
    call.items[1].origin_xy = None
    assert call() == call.lib.INVALID_ARGUMENT
    assert "insertion 1" in call.error(), call.error()
    call = _Call()
    call.items[3].num_misses = 2                      # misses_xyz is null
    assert call() == call.lib.INVALID_ARGUMENT
    assert "insertion 3" in call.error(), call.error()
    call = _Call()
    call.items[2].num_returns = -1
    assert call() == call.lib.INVALID_ARGUMENT
    assert "insertion 2" in call.error(), call.error()


# ---- the plan -------------------------------------------------------------------------------
def _plan_case():
    """Three grids -- 16 x 16, 100 x 100 and 5 x 5 -- and seven interleaved insertions; the third
    insertion of the first grid reaches x = 10, two doublings beyond its 8 m."""
    rng = np.random.default_rng(5)
    limits = [dict(resolution=0.5, max_x=4.0, max_y=4.0, num_x_cells=16, num_y_cells=16),
              dict(resolution=0.1, max_x=5.0, max_y=5.0, num_x_cells=100, num_y_cells=100),
              dict(resolution=1.0, max_x=2.5, max_y=2.5, num_x_cells=5, num_y_cells=5)]

    def points(n, lo, hi):
        xyz = np.zeros((n, 3), np.float32)
        xyz[:, :2] = rng.uniform(lo, hi, (n, 2))
        return xyz

    far = points(6, -3.0, 3.0)
    far[4, 0] = 10.0
    insertions = [
        (0, (0.3, -0.2), points(9, -3.0, 3.0), None),
        (1, (0.0, 0.1), points(40, -4.0, 4.0), points(5, -4.5, 4.5)),
        (0, (-1.0, 1.0), points(7, -3.5, 3.5), points(3, -3.0, 3.0)),
        (2, (0.2, 0.2), points(4, -1.5, 1.5), None),
        (0, (0.5, 0.5), far, None),
        (1, (1.0, -1.0), points(33, -4.0, 4.0), None),
        (0, (2.0, 2.0), points(8, -6.0, 6.0), None),
    ]
    return limits, insertions


def test_plan_gives_the_rounds_and_the_limits_of_the_inserts_in_order():
    from cartographer_amd import grid_2d, synth
    limits, insertions = _plan_case()
    rounds, final = grid_2d.insert_batch_plan(limits, insertions)
    assert rounds == [0, 0, 1, 0, 2, 1, 3]
    hosts = [synth.ProbabilityGrid(l["resolution"], (l["max_x"], l["max_y"]), l["num_x_cells"],
                                   l["num_y_cells"]) for l in limits]
    sizes = []
    for grid, origin, returns, misses in insertions:
        hosts[grid].insert(origin, returns, misses)
        sizes.append(hosts[grid].limits["num_x_cells"])
    assert [sizes[k] for k in (0, 2, 4, 6)] == [16, 16, 64, 64]   # twice, at the third insertion
    assert final == [h.limits for h in hosts]
    assert final[1] == limits[1] and final[2] == limits[2]


def test_plan_refuses_a_grid_that_would_pass_2_30_cells():
    from cartographer_amd import _lib, grid_2d
    limits = [dict(resolution=0.001, max_x=8.0, max_y=8.0, num_x_cells=16384, num_y_cells=16384)]
    far = np.array([[1e6, 0.0, 0.0]], np.float32)
    try:
        grid_2d.insert_batch_plan(limits, [(0, (0.0, 0.0), None, None), (0, (0.0, 0.0), far, None)])
    except _lib.CmxError as e:
        assert e.status == _lib.INVALID_ARGUMENT and "insertion 1" in str(e)
    else:
        raise AssertionError("planned a grid beyond 2^30 cells")
