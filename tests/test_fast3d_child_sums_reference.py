"""The integer child sums of the fast 3D branch and bound, restated in numpy over int64, and the
CPU anchors of that restatement (no GPU).

tests/test_gpu_fast3d_child_sums.py compares what cmx_debug_fast3d_child_sums returns with
`child_sums` below.  The restatement follows SM3/fast_correlative_scan_matcher_3d.cc :223-241 (the
cell indices of a scan at every depth) and :332-355 (ScoreCandidates); the levels it reads are the
oracle's.  So that it is not pinned by the device code alone, this file holds it against the
oracle's own search: the score of the oracle's winning leaf bit for bit, the maximum over the
whole window, and -- on a stack with half-resolution levels -- the bound every level has to be
for the full-resolution candidates it stands for.  The declaration, export and ctypes mirror of the
debug entry are checked here too.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cmx_debug_fast3d_child_sums"
VOXEL_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("z", np.int32), ("value", np.uint16),
                        ("pad", np.uint16)])


# ---- the restatement ------------------------------------------------------------------------
class DenseLevel:
    """One precomputation level from the sparse (x, y, z, value) rows of the oracle's level()."""

    def __init__(self, sparse):
        sparse = np.asarray(sparse, np.int64).reshape(-1, 4)
        if sparse.shape[0] == 0:
            self.lo = np.zeros(3, np.int64)
            self.cells = np.zeros((1, 1, 1), np.int64)
            return
        self.lo = sparse[:, :3].min(0)
        dims = sparse[:, :3].max(0) - self.lo + 1
        self.cells = np.zeros((dims[2], dims[1], dims[0]), np.int64)
        r = sparse[:, :3] - self.lo
        self.cells[r[:, 2], r[:, 1], r[:, 0]] = sparse[:, 3]

    def value(self, index):
        """PrecomputationGrid3D::value of int64 [n,3] indices: 0 outside the stored cells."""
        r = np.asarray(index, np.int64) - self.lo
        dims = np.array(self.cells.shape[::-1], np.int64)
        inside = np.all((r >= 0) & (r < dims), axis=1)
        r = np.where(inside[:, None], r, 0)
        return np.where(inside, self.cells[r[:, 2], r[:, 1], r[:, 0]], 0)


def reduction_exponent(depth, full_resolution_depth):
    return max(0, depth - full_resolution_depth + 1)


def depth_indices(cells, window, depth, full_resolution_depth):
    """:223-241: the cell indices of a scan at `depth` from its full-resolution ones; `window` =
    (wxy, wxy, wz).  (numpy's >> on int64 is the arithmetic shift of the reference's ints.)"""
    e = reduction_exponent(depth, full_resolution_depth)
    w = np.asarray(window, np.int64)
    return ((np.asarray(cells, np.int64) - w) >> e) - ((-w) >> e)


def candidate_indices(cells, window, depth, full_resolution_depth, offset):
    """:332-355: the cells a candidate with `offset` at `depth` reads, int64 [n,3]."""
    e = reduction_exponent(depth, full_resolution_depth)
    return depth_indices(cells, window, depth, full_resolution_depth) + \
        (np.asarray(offset, np.int64) >> e)


def candidate_sum(levels, full_resolution_depth, cells, window, depth, offset):
    index = candidate_indices(cells, window, depth, full_resolution_depth, offset)
    return int(levels[depth].value(index).sum())


def child_offsets(node):
    """The eight children of node (level, ox, oy, oz): k = x + 2 y + 4 z, half a step apart."""
    level, o = int(node[0]), np.asarray(node[1:4], np.int64)
    half = 1 << (level - 1)
    return [o + half * np.array([k & 1, k >> 1 & 1, k >> 2 & 1], np.int64) for k in range(8)]


def child_sums(levels, full_resolution_depth, cells, wxy, wz, node):
    """int64 [8]: the sums ScoreCandidates gives the eight children of `node`."""
    window = (wxy, wxy, wz)
    return np.array([candidate_sum(levels, full_resolution_depth, cells, window, int(node[0]) - 1,
                                   o) for o in child_offsets(node)], np.int64)


def to_probability_f32(total, n):
    """PrecomputationGrid3D::ToProbability(sum / float(N)) in f32, the reference's order."""
    f = np.float32
    return f(0.1) + (f(total) / f(n)) * f((f(1.0) - f(0.1) - f(0.1)) / f(255.0))


def box_voxels(lo, extent, seed):
    """A solid box of voxels, values random in 1 .. 32767 with both ends present (they quantise
    to 0 and 255); a single voxel holds 32767."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*[np.arange(lo[k], lo[k] + extent[k]) for k in range(3)], indexing="ij")
    v = np.zeros(x.size, VOXEL_DTYPE)
    v["x"], v["y"], v["z"] = x.ravel(), y.ravel(), z.ravel()
    v["value"] = rng.integers(1, 32768, x.size)
    v["value"][0] = 1
    v["value"][-1] = 32767
    return v


# ---- the entry: declared, exported, mirrored -------------------------------------------------
def test_debug_header_declares_the_entry_and_the_loader_mirrors_it():
    from cartographer_amd import _lib
    text = open(os.path.join(ROOT, "include", "cartographer_mi355x_debug.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cmx_status\s+%s\s*\((.*?)\)\s*;" % ENTRY, stripped, re.S)
    assert m, f"{ENTRY} is not declared"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 11
    # not part of the drop-in boundary
    assert ENTRY not in open(os.path.join(ROOT, "include", "cartographer_mi355x.h")).read()
    assert ENTRY in _lib.DEBUG_SYMBOLS and ENTRY not in _lib.EXPORTED_SYMBOLS
    L = _lib.lib()
    assert hasattr(L, ENTRY), f"{ENTRY} is not exported"
    assert len(getattr(L, ENTRY).argtypes) == 11
    assert C.sizeof(_lib.DebugFast3DNode) == 16
    assert [f[0] for f in _lib.DebugFast3DNode._fields_] == ["level", "ox", "oy", "oz"]
    for name, value in (("OCT_BUFFER", 0), ("OCT_PLAIN", 1), ("WINDOWS", 2), ("BYTES", 3),
                        ("FAMILY", 4)):
        assert re.search(r"CMX_FAST3D_SUMS_%s\s*=\s*%d\b" % (name, value), stripped)


def test_null_arguments_are_refused_before_anything_is_read():
    from cartographer_amd import _lib
    node = (_lib.DebugFast3DNode * 1)()
    node[0].level = 1
    cells = np.zeros((1, 3), np.int32)
    sums, path = np.zeros(8, np.int32), np.zeros(1, np.int32)
    L = _lib.lib()
    # (no matcher exists without a device: the null handle is the first check)
    assert L.cmx_debug_fast3d_child_sums(None, cells.ctypes.data, 1, 1, 1, node, 1, 0, 1,
                                         sums.ctypes.data, path.ctypes.data) == \
        _lib.INVALID_ARGUMENT


# ---- anchors ---------------------------------------------------------------------------------
def _shell_scene(seed, lo, extent):
    """Voxels of a hollow box with random values and points near the centres of some of them."""
    rng = np.random.default_rng(seed)
    v = box_voxels(lo, extent, seed)
    hi = np.asarray(lo) + np.asarray(extent) - 1
    on_shell = np.zeros(v.shape[0], bool)
    for k, name in enumerate("xyz"):
        on_shell |= (v[name] == lo[k]) | (v[name] == hi[k])
    v = v[on_shell]
    v["value"] = rng.integers(1, 32768, v.shape[0])
    return v, rng


def _cloud_on(v, rng, count, resolution, shift):
    """`count` points within 0.3 cells of voxel centres, moved by -shift (so that a search from
    `shift` finds them where the voxels are), as f32."""
    pick = rng.choice(v.shape[0], count, replace=False)
    centre = np.stack([v["x"][pick], v["y"][pick], v["z"][pick]], 1).astype(np.float64)
    p = (centre + rng.uniform(-0.3, 0.3, (count, 3))) * resolution - np.asarray(shift)
    return p.astype(np.float32)


def _full_resolution_cells(points, t0, resolution):
    """DiscretizeScan (:200-221) for an identity rotation, in f32: lround((p + t0) / resolution).
    The points lie away from half-integers, which the test asserts, so that the rounding of the
    division cannot decide a cell."""
    q = (points + np.asarray(t0, np.float32)) / np.float32(resolution)
    assert q.dtype == np.float32
    assert np.all(np.abs(q - np.floor(q) - 0.5) > 1e-2)
    return np.floor(q + np.float32(0.5)).astype(np.int64)


def _oracle_search(oracle, voxels, points, t0, resolution, depth, frd, window_xy, window_z):
    hist = np.zeros(8, np.float32)
    om = oracle.FastCorrelativeScanMatcher3D(resolution, voxels, resolution, voxels, hist, depth,
                                             frd, 0.0, 0.0, window_xy, window_z, 0.0)
    ident = [1.0, 0.0, 0.0, 0.0]
    ref = om.match(list(map(float, t0)) + ident, [0.0, 0.0, 0.0] + ident, ident, points,
                   points[::3].copy(), hist, 0.05)
    assert ref["found"] and ref["num_scans"] == 1
    levels = [DenseLevel(om.level(d)) for d in range(depth)]
    return ref, levels


def test_leaf_sum_of_the_restatement_is_the_oracles_winning_score():
    """One scan (angular window 0, identity orientations): at child depth 0 the restatement's sum
    for the oracle's winning translation gives the oracle's score bit for bit, and no offset of the
    window gives a higher one."""
    from oracle import pyoracle as oracle
    resolution = 0.1
    v, rng = _shell_scene(3, (-6, -5, -2), (12, 9, 5))
    true_shift = np.array([0.2, -0.1, 0.1])
    points = _cloud_on(v, rng, 60, resolution, true_shift)
    t0 = np.array([0.0, 0.1, 0.0], np.float32)            # two cells in x, two in y, one in z off
    wxy, wz = 3, 2
    ref, levels = _oracle_search(oracle, v, points, t0, resolution, 3, 3, wxy * resolution,
                                 wz * resolution)
    cells = _full_resolution_cells(points, t0, resolution)
    n = points.shape[0]
    offset = np.rint((ref["pose"][:3] - t0.astype(np.float64)) / resolution).astype(np.int64)
    assert np.all(np.abs(offset) <= (wxy, wxy, wz))
    window = (wxy, wxy, wz)
    total = candidate_sum(levels, 3, cells, window, 0, offset)
    score = to_probability_f32(total, n)
    assert score.dtype == np.float32
    assert score == np.float32(ref["score"]), (total, score, ref["score"])
    best = max(candidate_sum(levels, 3, cells, window, 0, (x, y, z))
               for x in range(-wxy, wxy + 1) for y in range(-wxy, wxy + 1)
               for z in range(-wz, wz + 1))
    assert best == total and total > 0
    # the same leaf as child k of its parent at level 1, through child_sums
    parent = offset - ((offset + np.array(window)) & 1)
    k = int(((offset - parent) * (1, 2, 4)).sum())
    assert child_sums(levels, 3, cells, wxy, wz, (1, *parent))[k] == total


@pytest.mark.parametrize("depth,frd", [(5, 2), (4, 1)])
def test_sums_above_the_full_resolution_levels_bound_the_leaves_they_stand_for(depth, frd):
    """Half-resolution levels: the restatement's sum of a candidate at depth c >= frd (offsets
    as the search generates them, -window + i 2^c) is at least the leaf sum of every
    full-resolution offset the candidate covers -- and the oracle's winning score is met at
    depth 0, as above."""
    from oracle import pyoracle as oracle
    resolution = 0.1
    v, rng = _shell_scene(9, (-7, -3, -4), (11, 10, 6))
    points = _cloud_on(v, rng, 50, resolution, (0.1, 0.2, -0.1))
    t0 = np.array([0.0, 0.0, 0.0], np.float32)
    wxy, wz = 5, 3
    window = np.array([wxy, wxy, wz])
    ref, levels = _oracle_search(oracle, v, points, t0, resolution, depth, frd,
                                 wxy * resolution, wz * resolution)
    cells = _full_resolution_cells(points, t0, resolution)
    offset = np.rint(ref["pose"][:3] / resolution).astype(np.int64)
    total = candidate_sum(levels, frd, cells, window, 0, offset)
    assert to_probability_f32(total, points.shape[0]) == np.float32(ref["score"])
    checked = 0
    for c in range(frd, depth):
        step = 1 << c
        tight = 0
        for i in np.ndindex(*[int(-(-(2 * w + 1) // step)) for w in window]):
            o = -window + np.array(i) * step
            bound = candidate_sum(levels, frd, cells, window, c, o)
            covered = max(candidate_sum(levels, frd, cells, window, 0, o + np.array(d))
                          for d in np.ndindex(step, step, step))
            assert bound >= covered, (c, o, bound, covered)
            tight += bound > 0
            checked += 1
        assert tight > 0, f"depth {c}: every bound is 0, the scene says nothing"
    assert checked >= depth - frd


@pytest.mark.parametrize("wxy", [5, 6])
def test_one_voxel_one_point_every_position_is_bounded(wxy):
    """The same bound where it is sharpest: one occupied voxel, one point, the point at every
    cell of a line through the voxel (negative and positive, odd and even).  A level's cell is
    non-zero only in the few cells around the voxel, so an index that is off by one -- a shift
    that rounds towards zero, a window term left out -- reads 0 where a covered leaf reads the
    voxel."""
    from oracle import pyoracle as oracle
    depth, frd, wz = 5, 2, 3
    window = np.array([wxy, wxy, wz])
    hist = np.zeros(8, np.float32)
    for voxel in ((-3, 2, -1), (4, -5, 2)):
        v = np.zeros(1, VOXEL_DTYPE)
        v["x"], v["y"], v["z"] = voxel
        v["value"] = 32767
        om = oracle.FastCorrelativeScanMatcher3D(0.1, v, 0.1, v, hist, depth, frd, 0.0, 0.0,
                                                 0.1 * wxy, 0.1 * wz, 0.0)
        levels = [DenseLevel(om.level(d)) for d in range(depth)]
        assert levels[0].value([voxel])[0] == 255
        hits = 0
        for axis in range(3):
            for at in range(-24, 25):
                # (on the other two axes the offset -window puts the point on the voxel)
                cell = np.array([voxel], np.int64) + window
                cell[0, axis] = at
                for c in range(frd, depth):
                    step = 1 << c
                    for i in range(-(-(2 * window[axis] + 1) // step)):
                        o = -window.copy()
                        o[axis] += i * step
                        bound = candidate_sum(levels, frd, cell, window, c, o)
                        covered = 0
                        for d in range(step):
                            leaf = o.copy()
                            leaf[axis] += d
                            covered = max(covered,
                                          candidate_sum(levels, frd, cell, window, 0, leaf))
                        assert bound >= covered, (voxel, axis, at, c, o, bound, covered)
                        hits += covered > 0
        assert hits > 0
