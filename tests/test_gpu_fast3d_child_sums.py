"""The eight integer child sums of the fast 3D branch and bound on every load path, against plain
integer sums.

cmx_debug_fast3d_child_sums runs the device functions of the search (ChildSums3D / FamilySums3D
with their reductions) on nodes, cells and live masks a test chooses and says which loads
produced every row.  The expectation is numpy over int64 on the ORACLE's levels
(test_fast3d_child_sums_reference.py, anchored there on the CPU); no device output enters it.
Every comparison is assert_array_equal on integers: there are no tolerances in this file.

Paths (CMX_FAST3D_SUMS_*): 0 oct words through a buffer resource (default), 2 four 8-byte windows
per point (fast3d_no_oct, child cells at most 4 apart), 3 a byte load per child cell
(fast3d_byte_loads; fast3d_no_oct with child cells 8 or more apart), 4 the family loop.  Path 1
(oct arrays of 2 GB or more) is not reachable at test sizes.

The end-to-end additions at the bottom (low-resolution clouds around the 2048-point chunk of the
leaf verification, a high-resolution cloud of 65 537 points) keep the bars of test_gpu_3d.py.
"""
import itertools

import numpy as np
import pytest

from test_fast3d_child_sums_reference import (DenseLevel, box_voxels, candidate_indices,
                                              child_offsets, child_sums, reduction_exponent)

pytestmark = pytest.mark.gpu

STACKS = [(2, 1), (4, 2), (5, 3), (6, 6), (6, 4), (8, 3)]
# lowest corner per axis: negative odd, negative even, zero, positive odd -- each on every axis;
# extents 1x1x1, 3x5x2, 17x9x4 and a row of 40 cells (longer than an 8-byte window)
BOXES = [((-7, -4, 0), (1, 1, 1)), ((-8, 3, -5), (3, 5, 2)), ((0, -9, 5), (17, 9, 4)),
         ((5, 0, -4), (40, 3, 2))]
WXY, WZ = 5, 3
WINDOW = np.array([WXY, WXY, WZ], np.int64)
COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025]
MODES = {"default": {}, "no_oct": dict(fast3d_no_oct=1), "bytes": dict(fast3d_byte_loads=1)}
OCT, WINDOWS, BYTES, FAMILY = 0, 2, 3, 4
SENTINEL = -77


@pytest.fixture(scope="module")
def sm3():
    from cartographer_amd import _lib, scan_matching_3d
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching_3d


def child_stride(child_depth, frd):
    """Cells between the two x positions of a node's children at their level."""
    return 1 << min(child_depth, frd - 1)


def expected_path(mode, child_depth, frd):
    if mode == "bytes":
        return BYTES
    if mode == "no_oct":
        return WINDOWS if child_stride(child_depth, frd) <= 4 else BYTES
    return OCT


OPTIONS = dict(min_rotational_score=0.0, min_low_resolution_score=0.0,
               linear_xy_search_window=0.5, linear_z_search_window=0.3, angular_search_window=0.0)
_levels = {}


def oracle_levels(oracle, key, voxels, depth, frd):
    """The oracle's precomputation stack of a scene, computed once per module and left alone."""
    if key not in _levels:
        om = oracle.FastCorrelativeScanMatcher3D(
            0.1, voxels, 0.1, voxels, np.zeros(8, np.float32), depth, frd,
            OPTIONS["min_rotational_score"], OPTIONS["min_low_resolution_score"],
            OPTIONS["linear_xy_search_window"], OPTIONS["linear_z_search_window"],
            OPTIONS["angular_search_window"])
        _levels[key] = [DenseLevel(om.level(d)) for d in range(depth)]
    return _levels[key]


def device_matcher(sm3, voxels, depth, frd):
    return sm3.FastCorrelativeScanMatcher3D(0.1, voxels, 128, 0.1, voxels, np.zeros(8, np.float32),
                                            branch_and_bound_depth=depth,
                                            full_resolution_depth=frd, **OPTIONS)


def border_cells(node, frd, lo, dims, rng):
    """Full-resolution cells whose lower child position (k = 0) of `node` lies, per axis, at the
    cells -s - 1, -s, -1, 0, n - s - 1, n - s, n - 1 and n of the level's array (lo, dims) --
    s the child stride -- in every combination: oct indices -1, 0, q - 1 and q, both children
    outside on either side, one inside and one outside, the last column, row and slab."""
    level = int(node[0])
    c = level - 1
    e = reduction_exponent(c, frd)
    s = child_stride(c, frd)
    per_axis = []
    for k in range(3):
        n = int(dims[k])
        targets = sorted({-s - 1, -s, -1, 0, n - s - 1, n - s, n - 1, n})
        # index at depth c wanted: t + lo - (o >> e); the full-resolution cells that give it
        u = np.array(targets, np.int64) + int(lo[k]) - (int(node[1 + k]) >> e)
        per_axis.append(((u + ((-int(WINDOW[k])) >> e)) << e) + int(WINDOW[k]))
    cells = np.array(list(itertools.product(*per_axis)), np.int64)
    return cells + rng.integers(0, 1 << e, cells.shape)


def assert_faces_and_inside(node, frd, cells, lo, dims):
    """A test bug otherwise: the children of `node` look outside the level's array on each of its
    six faces, and inside it."""
    c = int(node[0]) - 1
    lo, dims = np.asarray(lo, np.int64), np.asarray(dims, np.int64)
    below, above, inside = np.zeros(3, bool), np.zeros(3, bool), False
    for o in child_offsets(node):
        r = candidate_indices(cells, WINDOW, c, frd, o) - lo
        others_in = [np.all((np.delete(r, k, 1) >= 0) & (np.delete(r, k, 1) < np.delete(dims, k)),
                            axis=1) for k in range(3)]
        for k in range(3):
            below[k] |= bool(np.any((r[:, k] < 0) & others_in[k]))
            above[k] |= bool(np.any((r[:, k] >= dims[k]) & others_in[k]))
        inside |= bool(np.any(np.all((r >= 0) & (r < dims), axis=1)))
    assert below.all() and above.all() and inside, (node, below, above, inside)


def scene_nodes(depth):
    """Per level: the window's corner, a node whose upper children leave the window (their sums
    are compared all the same), and one at an odd offset, negative on one axis."""
    nodes = []
    for level in range(1, depth):
        half = 1 << (level - 1)
        nodes += [(level, -WXY, -WXY, -WZ), (level, WXY - half + 1, WXY, WZ - half + 1),
                  (level, 1, -3, 2)]
    return nodes


def scene_cells(nodes, frd, box, box_of_level, rng, random_count=160):
    """Border cells of every node, random cells over the box plus twice the window, and a few
    at +-2^20 (far outside: they read 0 and must not wrap)."""
    lo, extent = np.array(box[0]), np.array(box[1])
    parts = [border_cells(nd, frd, *box_of_level(nd[0] - 1), rng) for nd in nodes]
    parts.append(rng.integers(lo - 2 * WINDOW - 2, lo + extent + 2 * WINDOW + 2,
                              (random_count, 3)))
    far = 1 << 20
    parts.append(np.array([(far, 0, 0), (-far, 0, 0), (0, far, 0), (0, -far, 0), (1, 2, far),
                           (1, 2, -far), (far, far, far), (-far, -far, -far)], np.int64))
    cells = np.concatenate(parts)
    return cells[rng.permutation(cells.shape[0])]


def expect(levels, frd, cells, nodes, wxy=WXY, wz=WZ):
    return np.stack([child_sums(levels, frd, cells, wxy, wz, nd) for nd in nodes]).astype(np.int32)


# ---- geometry, depths, borders: every child level of every stack on paths 0, 2 and 3 ----------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("depth,frd", STACKS)
def test_child_sums_of_every_level_at_the_borders(sm3, oracle, debug, depth, frd, mode):
    debug(**MODES[mode])
    nodes = scene_nodes(depth)
    for b, box in enumerate(BOXES):
        voxels = box_voxels(*box, seed=b)
        levels = oracle_levels(oracle, (b, depth, frd), voxels, depth, frd)
        gm = device_matcher(sm3, voxels, depth, frd)
        rng = np.random.default_rng(100 * depth + 10 * frd + b)
        cells = scene_cells(nodes, frd, box, gm.level_box, rng)
        for nd in nodes:
            assert_faces_and_inside(nd, frd, cells, *gm.level_box(nd[0] - 1))
        sums, path = gm.debug_child_sums(cells, WXY, WZ, nodes)
        np.testing.assert_array_equal(sums, expect(levels, frd, cells, nodes),
                                      err_msg=f"box {box}")
        np.testing.assert_array_equal(path, [expected_path(mode, nd[0] - 1, frd) for nd in nodes])
        assert sums.max() > 0


def test_no_oct_reaches_the_byte_path_only_where_child_cells_are_eight_apart():
    """(6, 4) and (6, 6) without oct words: the only way into path 3 without its switch."""
    assert [expected_path("no_oct", c, 4) for c in range(5)] == [2, 2, 2, 3, 3]
    assert [expected_path("no_oct", c, 6) for c in range(5)] == [2, 2, 2, 3, 3]
    assert [expected_path("no_oct", c, 3) for c in range(7)] == [2] * 7


# ---- point counts: idle lanes, the tails of the unrolled loops, a lane's second iteration -----
@pytest.mark.parametrize("mode", list(MODES))
def test_child_sums_at_every_point_count(sm3, oracle, debug, mode):
    debug(**MODES[mode])
    box_index = 2
    box = BOXES[box_index]
    voxels = box_voxels(*box, seed=box_index)
    for depth, frd in ((5, 3), (6, 4)):
        levels = oracle_levels(oracle, (box_index, depth, frd), voxels, depth, frd)
        gm = device_matcher(sm3, voxels, depth, frd)
        nodes = scene_nodes(depth)
        rng = np.random.default_rng(7 + depth)
        pool = scene_cells(nodes, frd, box, gm.level_box, rng)
        assert pool.shape[0] >= max(COUNTS)
        for n in COUNTS:
            cells = pool[:n]
            sums, path = gm.debug_child_sums(cells, WXY, WZ, nodes)
            np.testing.assert_array_equal(sums, expect(levels, frd, cells, nodes),
                                          err_msg=f"n = {n}")
            np.testing.assert_array_equal(path,
                                          [expected_path(mode, nd[0] - 1, frd) for nd in nodes])
            # families of 2 and of 8 at the same counts (the n % 2 tail of the family loop)
            for level in range(1, depth):
                for size in (2, 8):
                    family = family_of((level + 1, -WXY, 1, -WZ), range(size))
                    check_family(gm, levels, frd, cells, family, (1 << size) - 1,
                                 FAMILY if mode == "default" else None, mode)


# ---- families ---------------------------------------------------------------------------------
def family_of(parent, members):
    """Children `members` (k = x + 2 y + 4 z) of `parent` as nodes: one level, half a parent step
    apart -- what a parent keeps."""
    offsets = child_offsets(parent)
    return [(parent[0] - 1, *map(int, offsets[k])) for k in members]


def check_family(gm, levels, frd, cells, family, live, path_expected, mode, wxy=WXY, wz=WZ):
    size = len(family)
    sums = np.full((size, 8), SENTINEL, np.int32)
    path = np.full(size, SENTINEL, np.int32)
    gm.debug_child_sums(cells, wxy, wz, family, as_family=True, live_mask=live, sums=sums,
                        path=path)
    single, single_path = gm.debug_child_sums(cells, wxy, wz, family)
    want = expect(levels, frd, cells, family, wxy, wz)
    for m in range(size):
        if live >> m & 1:
            np.testing.assert_array_equal(sums[m], want[m], err_msg=f"member {m} of {family}")
            np.testing.assert_array_equal(sums[m], single[m])
            # a family the loop does not take goes member by member: their own paths
            assert path[m] == (path_expected if path_expected is not None else single_path[m])
            assert single_path[m] == expected_path(mode, family[m][0] - 1, frd)
        else:
            assert np.all(sums[m] == SENTINEL) and path[m] == SENTINEL, f"dead member {m} written"


def live_masks(size):
    full = (1 << size) - 1
    return [full, full & ~1, full & ~(1 << (size - 1)), full & 0x55, full & 0xaa, 1,
            1 << (size - 1), 1 << (size // 2)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", range(2, 9))
def test_families_of_every_size_and_live_mask(sm3, oracle, debug, size, mode):
    """F = 2 .. 8 members at every level of two stacks; all alive, the first / the last /
    alternating members dead, one alone alive.  Default: the family loop (path 4).  Without oct
    words or with byte loads the family is refused and its live members go one by one."""
    debug(**MODES[mode])
    box_index = 2
    box = BOXES[box_index]
    voxels = box_voxels(*box, seed=box_index)
    rng = np.random.default_rng(size)
    for depth, frd in ((5, 3), (8, 3)):
        levels = oracle_levels(oracle, (box_index, depth, frd), voxels, depth, frd)
        gm = device_matcher(sm3, voxels, depth, frd)
        for level in range(1, depth):
            members = sorted(rng.choice(8, size, replace=False).tolist())
            family = family_of((level + 1, -WXY + 2 * (level % 2), -3, -WZ), members)
            cells = scene_cells(family[:1] + family[-1:], frd, box, gm.level_box, rng, 300)
            cells = cells[:1023 if level % 2 else 600]
            for live in live_masks(size):
                check_family(gm, levels, frd, cells, family, live,
                             FAMILY if mode == "default" else None, mode)


# ---- long, saturated clouds: the 16-bit ceiling of the packed sums and the second pass ---------
BLOCK_LO, BLOCK = -12, 24
LONG_STACK = (4, 2)
LONG_W = (2, 1)


def block_voxels(shell):
    """24^3 voxels of 32767 (u8 255); with `shell` inside four more layers of lower, random
    values on every side."""
    if not shell:
        v = box_voxels((BLOCK_LO,) * 3, (BLOCK,) * 3, seed=0)
        v["value"] = 32767
        return v
    v = box_voxels((BLOCK_LO - 4,) * 3, (BLOCK + 8,) * 3, seed=5)
    core = np.ones(v.shape[0], bool)
    for name in "xyz":
        core &= (v[name] >= BLOCK_LO) & (v[name] < BLOCK_LO + BLOCK)
    v["value"] = np.where(core, 32767, np.minimum(v["value"], 20000))
    return v


LONG_NODES = [(1, -2, -2, -1), (2, -2, -2, -1), (3, -2, -2, -1), (1, 1, 0, -1)]
SHELL_NODES = [(1, 1, 0, 1), (2, 0, 1, 0), (3, -2, -2, -1)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [65536, 65537, 70001])
def test_saturated_cloud_at_the_ceiling_of_the_packed_sums(sm3, oracle, debug, n, mode):
    """Every cell read is 255 and every lane has 256 points in its first pass: the packed 16-bit
    halves reach 256 * 255 = 65 280; from 65 537 points on the second widening pass runs too.
    Every child sum is exactly 255 n.  Families: the loop takes 65 536 points (path 4) and
    refuses 65 537 (the members then come from path 0, same values).  (A loop that never widened
    would still pass 65 537 -- one lane with 257 points, 257 * 255 = 65 535 -- and fails 70 001.)"""
    debug(**MODES[mode])
    depth, frd = LONG_STACK
    voxels = block_voxels(False)
    levels = oracle_levels(oracle, ("block", depth, frd), voxels, depth, frd)
    gm = device_matcher(sm3, voxels, depth, frd)
    cells = np.random.default_rng(n).integers(-6, 6, (n, 3))      # inside by more than the window
    want = expect(levels, frd, cells, LONG_NODES, *LONG_W)
    assert np.all(want == 255 * n)
    sums, path = gm.debug_child_sums(cells, *LONG_W, LONG_NODES)
    np.testing.assert_array_equal(sums, want)
    np.testing.assert_array_equal(path, [expected_path(mode, nd[0] - 1, frd) for nd in LONG_NODES])
    for members in (range(8), (1, 4, 6)):
        family = family_of((2, -2, -2, -1), members)
        taken = mode == "default" and n <= 65536
        check_family(gm, levels, frd, cells, family, (1 << len(family)) - 1,
                     FAMILY if taken else None, mode, *LONG_W)


@pytest.mark.parametrize("mode", list(MODES))
def test_long_cloud_at_the_edge_of_the_block_gives_eight_different_sums(sm3, oracle, debug, mode):
    """The same block inside a shell of lower values, the cloud in its upper corner: the upper
    children read the shell, the eight sums differ -- a sum that lands in its neighbour's half of
    a packed word, or a pass that is dropped, shows."""
    debug(**MODES[mode])
    depth, frd = LONG_STACK
    voxels = block_voxels(True)
    levels = oracle_levels(oracle, ("shell", depth, frd), voxels, depth, frd)
    gm = device_matcher(sm3, voxels, depth, frd)
    n = 65537
    cells = np.random.default_rng(1).integers(4, 13, (n, 3))
    want = expect(levels, frd, cells, SHELL_NODES, *LONG_W)
    assert all(len(set(row.tolist())) == 8 for row in want)
    sums, path = gm.debug_child_sums(cells, *LONG_W, SHELL_NODES)
    np.testing.assert_array_equal(sums, want)
    np.testing.assert_array_equal(path,
                                  [expected_path(mode, nd[0] - 1, frd) for nd in SHELL_NODES])
    family = family_of((2, -2, -2, -1), range(8))
    check_family(gm, levels, frd, cells[:65536], family, 0xff,
                 FAMILY if mode == "default" else None, mode, *LONG_W)
    check_family(gm, levels, frd, cells, family, 0xbd, None, mode, *LONG_W)


# ---- arguments ----------------------------------------------------------------------------------
def test_invalid_arguments(sm3):
    import ctypes as C
    from cartographer_amd import _lib
    gm = device_matcher(sm3, box_voxels(*BOXES[1], seed=1), 4, 2)
    cells = np.zeros((3, 3), np.int32)

    def refused(nodes, **kw):
        with pytest.raises(_lib.CmxError) as e:
            gm.debug_child_sums(kw.pop("cells", cells), WXY, WZ, nodes, **kw)
        assert e.value.status == _lib.INVALID_ARGUMENT

    refused([(0, 0, 0, 0)])                                   # level outside [1, depth - 1]
    refused([(4, 0, 0, 0)])
    refused([(1, 0, 0, 0), (2, 0, 0, 0)], as_family=True)     # a family of two levels
    refused([(1, 0, 0, 0)], as_family=True)                   # sizes outside 2 .. 8
    refused([(1, k, 0, 0) for k in range(9)], as_family=True)
    refused([(1, 0, 0, 0)], cells=np.zeros((0, 3), np.int32))  # num_points < 1
    node = (_lib.DebugFast3DNode * 1)()
    node[0].level = 1
    sums, path = np.zeros(8, np.int32), np.zeros(1, np.int32)
    good = [gm._h, cells.ctypes.data, 3, WXY, WZ, node, 1, 0, 1, sums.ctypes.data,
            path.ctypes.data]
    for at in (0, 1, 5, 9, 10):
        args = list(good)
        args[at] = None
        assert _lib.lib().cmx_debug_fast3d_child_sums(*args) == _lib.INVALID_ARGUMENT
    assert _lib.lib().cmx_debug_fast3d_child_sums(*good) == _lib.OK


# ---- end to end against the oracle ---------------------------------------------------------------
def _assert_result(ref, got):
    assert (got is not None) == ref["found"]
    if got is None:
        return
    assert np.float32(got["score"]) == np.float32(ref["score"])
    assert np.float32(got["rotational_score"]) == np.float32(ref["rotational_score"])
    assert np.float32(got["low_resolution_score"]) == np.float32(ref["low_resolution_score"])
    pose = got["pose_estimate"]
    np.testing.assert_array_equal(np.array(list(pose.translation) + list(pose.rotation)),
                                  ref["pose"])


@pytest.fixture(scope="module")
def room(synth):
    """A small room at 0.1 m / 0.45 m and one dense scan of it (65 792 points), made once."""
    grid, world = synth.make_submap_3d(21, 0.1, (6.0, 5.0, 3.0), 3, 8, 64)
    low, _ = synth.make_submap_3d(21, 0.45, (6.0, 5.0, 3.0), 3, 8, 64)
    pos = world.free_position(5, 0.6)
    return dict(vox=grid.voxels(), low_vox=low.voxels(), grid_size=grid.grid_size, pos=pos,
                sparse=world.scan(pos, 0.0, 70, 64, seed=3),
                dense=world.scan(pos, 0.0, 257, 256, seed=3))


IDENT = [1.0, 0.0, 0.0, 0.0]


def _search_both(sm3, oracle, room, node, hi, lo, min_score, **opt):
    hist = np.zeros(8, np.float32)
    om = oracle.FastCorrelativeScanMatcher3D(
        0.1, room["vox"], 0.45, room["low_vox"], hist, opt["branch_and_bound_depth"],
        opt["full_resolution_depth"], opt["min_rotational_score"],
        opt["min_low_resolution_score"], opt["linear_xy_search_window"],
        opt["linear_z_search_window"], opt["angular_search_window"])
    ref = om.match(node + IDENT, [0.0, 0.0, 0.0] + IDENT, IDENT, hi, lo, hist, min_score)
    gm = sm3.FastCorrelativeScanMatcher3D(0.1, room["vox"], room["grid_size"], 0.45,
                                          room["low_vox"], hist, **opt)
    got = gm.match(sm3.Rigid3d(tuple(node)), sm3.Rigid3d(), sm3.TrajectoryNodeData(hi, lo, hist),
                   min_score)
    return ref, got


@pytest.mark.parametrize("n_low", [2047, 2048, 2049, 4097])
def test_low_resolution_clouds_around_the_verification_chunk(sm3, oracle, room, n_low):
    """The leaf verification sums the low-resolution cloud in f32, in point order, across chunks
    of 2048 points.  min_low_resolution_score is put just above the low-resolution score of the
    best-scoring leaf, so that the verification decides: that leaf fails, a leaf with a lower
    score passes (asserted from the oracle's two results)."""
    pos = room["pos"]
    node = [pos[0] + 0.15, pos[1] - 0.1, pos[2] + 0.1]
    hi, lo = room["sparse"][::9].copy(), room["sparse"][:n_low].copy()
    assert lo.shape[0] == n_low
    opt = dict(branch_and_bound_depth=3, full_resolution_depth=2, min_rotational_score=0.0,
               min_low_resolution_score=0.0, linear_xy_search_window=0.3,
               linear_z_search_window=0.2, angular_search_window=0.0)
    first, got = _search_both(sm3, oracle, room, node, hi, lo, 0.2, **opt)
    assert first["found"]
    _assert_result(first, got)
    threshold = float(np.float32(first["low_resolution_score"])) + 1e-4
    ref, got = _search_both(sm3, oracle, room, node, hi, lo, 0.2,
                            **dict(opt, min_low_resolution_score=threshold))
    assert ref["found"] and ref["score"] < first["score"]        # a better-scoring leaf failed
    assert ref["low_resolution_score"] >= threshold > first["low_resolution_score"]
    _assert_result(ref, got)


@pytest.mark.parametrize("families", [True, False])
def test_search_with_a_high_resolution_cloud_of_65537_points(sm3, oracle, room, debug, families):
    """More than 256 points per lane in a full search: the second pass of the packed sums in every
    expansion, and families that the family loop refuses.  Depth 3, a window of two cells, one
    angular step either way (three scans).  The oracle's single-thread match of this takes 0.03 s
    on the CPU."""
    if not families:
        debug(fast3d_no_families=1)
    pos = room["pos"]
    node = [pos[0] + 0.1, pos[1] - 0.1, pos[2] + 0.0]
    hi, lo = room["dense"][:65537].copy(), room["dense"][::200].copy()
    assert hi.shape[0] == 65537
    opt = dict(branch_and_bound_depth=3, full_resolution_depth=2, min_rotational_score=0.0,
               min_low_resolution_score=0.3, linear_xy_search_window=0.2,
               linear_z_search_window=0.2, angular_search_window=0.012)
    ref, got = _search_both(sm3, oracle, room, node, hi, lo, 0.2, **opt)
    assert ref["found"] and ref["num_scans"] == 3
    _assert_result(ref, got)
