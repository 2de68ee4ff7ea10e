"""cmx_fast3d_create_batch: the fast-3D matchers of many submaps built by one chain of launches.
Every matcher of a batch must be, bit for bit, what the single create of its source returns:
levels with their bounds, searches with and without oct words, the raw grids the refinement reads.
Sources mix resident grids of unlike extents, voxel lists, a hand-made list with negative indices
and another resolution, an empty resident pair and empty lists."""
import ctypes as C
import gc
import math
import re

import numpy as np
import pytest

from test_gpu_fast3d_resident import (_histogram, _key, _nodes, _options, _raw_level,
                                      _resident_grids, _results)

pytestmark = pytest.mark.gpu

DEPTHS = [(8, 3), (5, 2), (1, 1), (3, 5)]     # (1, 1): level 0 only, no octs; (3, 5): no half level


@pytest.fixture(scope="module")
def sm3():
    from cartographer_amd import _lib, scan_matching_3d
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return scan_matching_3d


@pytest.fixture(scope="module")
def scene(sm3, synth):
    """Six sources and the world the first one was filled from."""
    from cartographer_amd import grid_3d
    from cartographer_amd._lib import VOXEL_DTYPE
    world, high_a, low_a = _resident_grids(synth, 21, num_sweeps=5)
    _, high_b, low_b = _resident_grids(synth, 24, num_sweeps=3)
    _, high_c, low_c = _resident_grids(synth, 25, num_sweeps=4)
    hand = np.zeros(3, VOXEL_DTYPE)
    hand["x"], hand["y"], hand["z"] = [-7, -2, 3], [-5, 4, -1], [-3, -3, 2]
    hand["value"] = [40000, 33000, 1200]
    none = np.zeros(0, VOXEL_DTYPE)
    empty = (grid_3d.HybridGridOnDevice(0.1), grid_3d.HybridGridOnDevice(0.45))
    sources = [
        (high_a, low_a, _histogram(21)),
        (high_b, low_b, _histogram(24)),
        (0.1, high_c.voxels(), high_c.grid_size, 0.45, low_c.voxels(), _histogram(25)),
        (0.2, hand, 128, 0.5, hand[:2].copy(), _histogram(26)),
        (empty[0], empty[1], _histogram(27)),
        (0.1, none, 128, 0.45, none, _histogram(28)),
    ]
    assert high_a.voxels().shape[0] != high_b.voxels().shape[0]
    return dict(world=world, seed=21, sources=sources, nodes=_nodes(sm3, world, 21))


def _single(sm3, source, opt):
    if len(source) == 3:
        return sm3.FastCorrelativeScanMatcher3D.from_device_grids(*source, **opt)
    return sm3.FastCorrelativeScanMatcher3D(*source, **opt)


def _assert_same_levels(a, b, depth, what):
    for d in range(depth):
        for x, y, name in zip(_raw_level(a, d), _raw_level(b, d), ("lo", "dims", "cells")):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: level {d} {name}")


def _assert_batch_equals_singles(sm3, scene, depth, frd, nodes):
    opt = _options(depth, frd)
    batch = sm3.fast3d_create_batch(scene["sources"], **opt)
    assert len(batch) == len(scene["sources"])
    for k, source in enumerate(scene["sources"]):
        single = _single(sm3, source, opt)
        _assert_same_levels(batch[k], single, depth, f"source {k}")
        # (depth 1 has no level to bound with: its full-submap search scores every candidate,
        # seconds per submap, so only the first source runs it)
        full = depth > 1 or k == 0
        got = [_key(r) for r in _results(sm3, batch[k], nodes, full)]
        assert got == [_key(r) for r in _results(sm3, single, nodes, full)], f"source {k}"
        if k == 0:
            assert any(g is not None for g in got)
    return batch


@pytest.mark.parametrize("depth,frd", DEPTHS)
@pytest.mark.parametrize("no_oct", [0, 1])
def test_mixed_batch_equals_the_single_creates(sm3, scene, debug, depth, frd, no_oct):
    debug(fast3d_no_oct=no_oct)
    _assert_batch_equals_singles(sm3, scene, depth, frd, scene["nodes"][:3 if depth > 1 else 1])


def test_searches_and_refinement_equal_the_single_creates(sm3, scene):
    opt = _options(8, 3)
    batch = sm3.fast3d_create_batch(scene["sources"], **opt)
    singles = [_single(sm3, source, opt) for source in scene["sources"]]
    nodes = scene["nodes"]
    assert len(nodes) == 8
    ra, rb = _results(sm3, batch[0], nodes), _results(sm3, singles[0], nodes)
    assert [_key(r) for r in ra] == [_key(r) for r in rb]
    found = [r is not None for r in ra]
    assert any(found) and not all(found)
    # One call over all eight nodes, against the first three and the hand-made submap.
    which = [0, 1, 2, 0, 3, 0, 2, 0]
    args = ([n[0] for n in nodes], [n[1] for n in nodes], [k % 2 == 1 for k in range(8)],
            [n[3] for n in nodes], [n[2] for n in nodes])
    pa, _ = sm3.fast3d_match_pairs([batch[w] for w in which], *args)
    pb, _ = sm3.fast3d_match_pairs([singles[w] for w in which], *args)
    assert [_key(r) for r in pa] == [_key(r) for r in pb]
    assert pa[0] is not None
    # CeresScanMatcher3D over the raw grids each matcher keeps: those of the batch lie in its slab.
    ceres = sm3.CeresScanMatcher3D([1.0, 6.0], 5.0, 4e2)
    start = [r["pose_estimate"] if r is not None else n[0] for r, n in zip(pa, nodes)]
    everything = [True] * 8
    qa, sa = ceres.refine_pairs([batch[w] for w in which], everything, start, args[4])
    qb, sb = ceres.refine_pairs([singles[w] for w in which], everything, start, args[4])
    assert qa == qb and sa == sb
    assert any(p != s for p, s in zip(qa, start))


def test_found_case_equals_the_oracle(sm3, oracle, scene):
    opt = _options(6, 3)
    high, low, hist = scene["sources"][0]
    a = sm3.fast3d_create_batch(scene["sources"][:3], **opt)[0]
    om = oracle.FastCorrelativeScanMatcher3D(0.1, high.voxels(), 0.45, low.voxels(), hist, 6, 3,
                                             0.9, 0.3, 1.5, 0.5, math.radians(20.0))
    node_pose, submap_pose, data, min_score = scene["nodes"][0]
    got = a.match(node_pose, submap_pose, data, min_score)
    ref = om.match(list(node_pose.translation) + list(node_pose.rotation),
                   list(submap_pose.translation) + list(submap_pose.rotation),
                   list(data.gravity_alignment), data.high_resolution_point_cloud,
                   data.low_resolution_point_cloud, data.rotational_scan_matcher_histogram,
                   min_score)
    assert ref["found"] and got is not None
    for key in ("score", "rotational_score", "low_resolution_score"):
        assert np.float32(got[key]) == np.float32(ref[key]), key
    p = got["pose_estimate"]
    np.testing.assert_array_equal(list(p.translation) + list(p.rotation), ref["pose"])


def test_matchers_outlive_their_sources_and_their_mates(sm3, synth):
    opt = _options(8, 3)
    world, high, low = _resident_grids(synth, 22, num_sweeps=3)
    _, high_b, low_b = _resident_grids(synth, 24, num_sweeps=2)
    hist = _histogram(22)
    lists = (0.1, high.voxels(), high.grid_size, 0.45, low.voxels(), hist)
    sources = [(high_b, low_b, hist), (high, low, hist), lists, lists, (high_b, low_b, hist),
               (high, low, hist)]
    batch = sm3.fast3d_create_batch(sources, **opt)
    nodes = _nodes(sm3, world, 22, 3)
    keep = (1, 3, 5)
    levels = {k: [_raw_level(batch[k], d) for d in range(8)] for k in keep}
    before = {k: [_key(r) for r in _results(sm3, batch[k], nodes)] for k in keep}
    assert any(r is not None for r in before[1])
    del sources, lists, high, low, high_b, low_b
    gc.collect()
    for k in (2, 0, 4):
        batch[k] = None                  # cmx_fast3d_destroy
    gc.collect()
    for k in keep:
        for d in range(8):
            for x, y in zip(_raw_level(batch[k], d), levels[k][d]):
                np.testing.assert_array_equal(x, y)
        assert [_key(r) for r in _results(sm3, batch[k], nodes)] == before[k]


def _trace(capfd):
    found = re.findall(r"fast3d_create_batch matchers=(\d+) chains=(\d+) launches=(\d+)",
                       capfd.readouterr().err)
    return [tuple(int(v) for v in f) for f in found]


def test_chains_of_two_and_a_launch_count_that_does_not_grow(sm3, scene, debug, capfd):
    """fast3d_create_chain = 2: the six sources go out as three chains of launches.  Without it,
    six sources take the launches two (one of either kind) take."""
    debug(fast3d_create_chain=2, host_trace=1)
    capfd.readouterr()
    _assert_batch_equals_singles(sm3, scene, 8, 3, scene["nodes"][:2])
    assert [t[:2] for t in _trace(capfd)] == [(6, 3)]
    debug(fast3d_create_chain=1)                    # and one by one
    _assert_batch_equals_singles(sm3, scene, 5, 2, scene["nodes"][:2])
    assert [t[:2] for t in _trace(capfd)] == [(6, 6)]
    debug(fast3d_create_chain=0)
    opt = _options(8, 3)
    six = sm3.fast3d_create_batch(scene["sources"], **opt)
    two = sm3.fast3d_create_batch(scene["sources"][1:3], **opt)
    (m6, c6, l6), (m2, c2, l2) = _trace(capfd)
    assert (m6, c6, m2, c2) == (6, 1, 2, 1) and l6 == l2
    # bounds: upload, launch, read-back; chain: upload, crop, zero, scatter, 7 levels, octs
    assert l6 == 3 + 4 + 7 + 1
    del six, two


def _records(sources):
    """The cmx_fast3d_source array of python sources (what fast3d_create_batch fills in)."""
    from cartographer_amd import _lib
    records = (_lib.Fast3DSource * len(sources))()
    keep = []
    for k, source in enumerate(sources):
        r = records[k]
        if len(source) == 3:
            r.high_resolution_grid, r.low_resolution_grid = source[0]._h, source[1]._h
        else:
            vox = np.ascontiguousarray(source[1], _lib.VOXEL_DTYPE)
            low = np.ascontiguousarray(source[4], _lib.VOXEL_DTYPE)
            keep += [vox, low]
            r.resolution, r.grid_size, r.low_resolution = source[0], source[2], source[3]
            r.voxels, r.num_voxels = (vox.ctypes.data if len(vox) else None), len(vox)
            r.low_resolution_voxels = low.ctypes.data if len(low) else None
            r.num_low_resolution_voxels = len(low)
        hist = np.ascontiguousarray(source[-1], np.float32)
        keep.append(hist)
        r.rotational_scan_matcher_histogram, r.histogram_size = hist.ctypes.data, len(hist)
    return records, keep


def test_all_or_nothing(sm3, scene):
    """A source of ambiguous kind in fourth place: nothing built, every out NULL, the index
    named; the same list without the damage builds right after."""
    from cartographer_amd import _lib
    L = _lib.lib()
    records, keep = _records(scene["sources"])
    num = len(records)
    opts = _lib.Fast3DOptions(*[_options(5, 2)[k] for k, _ in _lib.Fast3DOptions._fields_])
    out = (C.c_void_p * num)(*([0xdead] * num))
    records[3].high_resolution_grid = scene["sources"][0][0]._h       # voxel lists AND a grid
    assert L.cmx_fast3d_create_batch(C.byref(opts), records, num, 0, out) == _lib.INVALID_ARGUMENT
    assert "source 3" in L.cmx_last_error().decode()
    assert all(h is None for h in out)
    records[3].high_resolution_grid = None
    _lib.check(L.cmx_fast3d_create_batch(C.byref(opts), records, num, 0, out))
    assert all(h for h in out)
    lo, dims = np.zeros(3, np.int32), np.zeros(3, np.int32)
    _lib.check(L.cmx_fast3d_level_info(out[3], 0, lo.ctypes.data, dims.ctypes.data))
    assert list(lo) == [-7, -5, -3] and list(dims) == [11, 10, 6]
    for h in out:
        L.cmx_fast3d_destroy(h)
    if L.cmx_device_count() > 1:
        assert L.cmx_fast3d_create_batch(C.byref(opts), records, num, 1, out) == \
            _lib.INVALID_ARGUMENT
        assert "source 0" in L.cmx_last_error().decode() and all(h is None for h in out)
    del keep


def test_builder_with_batch_create_returns_the_same_constraints(sm3, scene):
    """Three submaps, two nodes, local and global constraints mixed: the constraint lists with
    and without batch_create are identical; with it nothing is built before the flush."""
    from cartographer_amd import constraint_builder as cb
    o = _options(6, 3)
    options = cb.ConstraintBuilderOptions3D(
        sampling_ratio=1.0, max_constraint_distance=50.0, min_score=0.15,
        global_localization_min_score=0.15, **o)
    submaps = []
    for source in scene["sources"][:3]:
        if len(source) == 3:
            high, low, hist = source
            source = (0.1, high.voxels(), high.grid_size, 0.45, low.voxels(), hist)
        submaps.append(cb.Submap3D(*source))
    nodes = scene["nodes"][:2]
    lists = {}
    for batch_create in (False, True):
        builder = cb.ConstraintBuilder3D(options, batch_create=batch_create)
        for j, (node_pose, submap_pose, data, _) in enumerate(nodes):
            for i, submap in enumerate(submaps):
                if (i + j) % 2 == 0:
                    builder.maybe_add_constraint((0, i), submap, (0, j), data, node_pose,
                                                 submap_pose)
                else:
                    builder.maybe_add_global_constraint((0, i), submap, (0, j), data,
                                                        node_pose.rotation, submap_pose.rotation)
        assert builder.num_scan_matchers() == (0 if batch_create else 3)
        out = []
        builder.when_done(out.extend)
        assert builder.num_scan_matchers() == 3
        lists[batch_create] = [(c.submap_id, c.node_id, c.zbar_ij, c.score, c.rotational_score,
                                c.low_resolution_score) for c in out]
    assert lists[True] == lists[False]
    assert len(lists[True]) >= 1
