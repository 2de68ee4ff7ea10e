"""Scenes, clouds, thresholds and edge cases of the fast 2D search over cost ranges other than a
probability grid's: shared by tests/test_reference_ref_fast2d_ranges.py (oracle against the
reference), tests/golden/make_fast2d_tsdf_golden.py (the reference's stored results) and
tests/test_gpu_fast2d_cost_ranges.py (device against oracle).  Everything is regenerated from
seeds; expected values are computed once per process and handed out read-only.

A TSDF2D's tsd plane is a Grid2D with min_correspondence_cost = -T, max_correspondence_cost = T
(T the truncation distance): a cell scores 1 - |tsd|, so scores lie in [1 - T, 1 + T] before
quantisation, min_s = 1 - T.
"""
import functools
import math

import numpy as np

from tsdf_helpers import tsdf_from_probability_grid

RES = 0.05
MAX_WEIGHT = 10.0
LIN, ANG = 1.0, math.radians(20.0)
OFFSET = (0.1, -0.05, 0.02)
# (seed, nx, ny, depth): square and non-square grids, depths 3 - 5
SCENES = ((11, 120, 120, 5), (12, 96, 150, 3), (13, 37, 53, 4))
TRUNCATIONS = (0.3, 0.1, 1.0)
# points per cloud: several wavefronts, one past two wavefronts, exactly one, a single point
CUTS = (300, 129, 64, 1)
# what a later lift of the max_correspondence_cost <= 1 restriction has to meet (CPU only)
UNSUPPORTED_TRUNCATION = 1.5


def f32(x):
    return float(np.float32(x))


def min_s_of(max_cc):
    """1.f - max_correspondence_cost, in f32 as every implementation forms it."""
    return float(np.float32(1.0) - np.float32(max_cc))


def score_scale_of(min_cc, max_cc):
    max_s = np.float32(1.0) - np.float32(min_cc)
    return float((max_s - np.float32(min_s_of(max_cc))) / np.float32(255.0))


class Scene:
    """One submap, its four clouds and their initial pose estimates."""

    def __init__(self, synth, orc, seed, nx, ny, depth):
        self.seed, self.nx, self.ny, self.depth = seed, nx, ny, depth
        self.cells, self.lim, world = synth.make_submap(seed, nx, ny, RES, 12, 400, 5.0, 0.01)
        self.cells.setflags(write=False)
        self.max_x, self.max_y = self.lim["max_x"], self.lim["max_y"]
        self.clouds, self.inits = [], []
        for k, cut in enumerate(CUTS):
            pose = world.free_pose(20 + k, 0.3)
            scan = world.scan(pose, 400, 5.0, 0.01, k)
            assert scan.shape[0] >= cut, (seed, k, scan.shape)
            cloud = np.ascontiguousarray(scan[:cut])
            cloud.setflags(write=False)
            self.clouds.append(cloud)
            self.inits.append([pose[0] + OFFSET[0], pose[1] + OFFSET[1], pose[2] + OFFSET[2]])
        self._orc = orc
        self._planes = {}

    def planes(self, truncation):
        """(tsd, weight) uint16 planes of the scene at this truncation distance."""
        if truncation not in self._planes:
            tsd, wgt = tsdf_from_probability_grid(self._orc, self.cells, RES, truncation,
                                                  MAX_WEIGHT, self.seed)
            tsd.setflags(write=False)
            wgt.setflags(write=False)
            self._planes[truncation] = (tsd, wgt)
        return self._planes[truncation]

    def centre(self):
        """Map-frame centre of the grid (cells[iy][ix]: x runs down the rows)."""
        return (self.max_x - 0.5 * RES * self.ny, self.max_y - 0.5 * RES * self.nx)


@functools.lru_cache(maxsize=None)
def _scene(synth, orc, index):
    return Scene(synth, orc, *SCENES[index])


def scene(synth, orc, index):
    return _scene(synth, orc, index)


def oracle_matcher(orc, cells, sc, depth, min_cc=None, max_cc=None):
    return orc.FastCorrelativeScanMatcher2D(cells, RES, sc.max_x, sc.max_y, depth, LIN, ANG,
                                            min_cc, max_cc)


@functools.lru_cache(maxsize=None)
def oracle_tsdf_matcher(synth, orc, index, truncation):
    sc = scene(synth, orc, index)
    return oracle_matcher(orc, sc.planes(truncation)[0], sc, sc.depth, -truncation, truncation)


def searches(sc):
    """(cloud index, full_submap) of the eight searches of a scene."""
    return [(k, full) for k in range(len(CUTS)) for full in (False, True)]


def run(matcher, sc, k, full, min_score):
    """One search of an oracle / reference matcher (same call shape)."""
    if full:
        return matcher.match_full_submap(sc.clouds[k], min_score)
    return matcher.match(sc.inits[k], sc.clouds[k], min_score)


def derive_thresholds(best_scores, min_s):
    """The thresholds of one (scene, range) from its own best scores, highest pruning power
    first: the midpoint between the two neighbouring ranked scores in the middle (found and
    not-found both occur), 1.0 (between a perfect TSDF hit, 1.00118 at truncation 0.3, and the
    scores of large clouds) and a value below min_s, where everything passes."""
    ranked = np.unique(np.asarray(best_scores, np.float32))
    assert ranked.size >= 2, ranked
    i = ranked.size // 2
    mid = f32(0.5 * (float(ranked[i - 1]) + float(ranked[i])))
    assert float(ranked[i - 1]) <= mid < float(ranked[i])     # (not found at ranked[i-1], found at ranked[i])
    return [mid, 1.0, f32(min_s - 0.05)]


@functools.lru_cache(maxsize=None)
def tsdf_expectations(synth, orc, index, truncation):
    """{(k, full, min_score): oracle result} for the derived thresholds of one (scene, T), and
    the thresholds.  Computed once; callers must not modify it."""
    sc = scene(synth, orc, index)
    m = oracle_tsdf_matcher(synth, orc, index, truncation)
    low = f32(min_s_of(truncation) - 0.05)
    base = {(k, full): run(m, sc, k, full, low) for k, full in searches(sc)}
    assert all(r["found"] for r in base.values())
    thresholds = derive_thresholds([r["score"] for r in base.values()], min_s_of(truncation))
    out = {}
    for (k, full), r in base.items():
        for t in thresholds:
            # the best score does not depend on the threshold: only the path to it does
            out[(k, full, t)] = r if t == low else run(m, sc, k, full, t)
    return out, thresholds


# ---- edge cases: ties at the floor --------------------------------------------------------------
OUTSIDE_CLOUD = np.array([[40.0, 40.0, 0.0], [40.1, 40.0, 0.0], [40.0, 40.1, 0.0]], np.float32)
NEAR_CLOUD = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0]], np.float32)
# nine points 0.1 m apart: at most one of them on a single known cell
LATTICE_CLOUD = np.array([[0.1 * i, 0.1 * j, 0.0] for i in range(3) for j in range(3)], np.float32)
EDGE_SCENE = 2           # the 37 x 53 grid


def edge_cases(synth, orc, truncation):
    """[(name, tsd plane, weight plane, init, cloud, [min_scores])] on the 37 x 53 scene:
    * outside: a three-point cloud at (40, 40) m, wholly outside the grid -- every windowed
      candidate ties at exactly min_s = 1 - T; found just below min_s, not found at min_s;
    * one_known: every cell unknown but the centre one (tsd 0), the cloud around the centre: at
      best one point of three on it, min_s + 128 * 2T / 255 / 3 -- above the floors, below the
      last threshold, min_s + T / 2.
    At T >= 1 also min_score -1.0 and 0.0 (min_s = 0 at T = 1: found with score 0.0 at -1.0)."""
    sc = scene(synth, orc, EDGE_SCENE)
    tsd, wgt = sc.planes(truncation)
    ms = np.float32(min_s_of(truncation))
    floors = [float(np.nextafter(ms, np.float32(-np.inf))), float(ms)]
    extra = [t for t in (-1.0, 0.0) if truncation >= 1.0 and t not in floors]
    lone_tsd = np.zeros_like(tsd)
    lone_wgt = np.zeros_like(wgt)
    lone_tsd[sc.ny // 2, sc.nx // 2] = orc.tsd_to_value(0.0, truncation)
    lone_wgt[sc.ny // 2, sc.nx // 2] = orc.weight_to_value(5.0, MAX_WEIGHT)
    cx, cy = sc.centre()
    return [("outside", tsd, wgt, [0.3, -0.2, 0.1], OUTSIDE_CLOUD, floors + extra),
            ("one_known", lone_tsd, lone_wgt, [cx + 0.2, cy - 0.15, 0.05], NEAR_CLOUD,
             floors + extra + [f32(float(ms) + 0.5 * truncation)])]


def same_result(got, want, what=""):
    """found equal, f32 score bit-equal, pose to 1e-12 (results as oracle dicts)."""
    assert bool(got["found"]) == bool(want["found"]), (what, got, want)
    if want["found"]:
        a, b = np.float32(got["score"]), np.float32(want["score"])
        assert a.view(np.uint32) == b.view(np.uint32), (what, got, want)
        np.testing.assert_allclose(np.asarray(got["pose"], np.float64)[:3], want["pose"], rtol=0,
                                   atol=1e-12, err_msg=str(what))
