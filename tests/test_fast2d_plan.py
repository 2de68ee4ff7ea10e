"""The plan of the fast 2D front end (cmx_debug_fast2d_plan) from the grids' geometry alone: host
arithmetic, no device.  It is the function the launch path asks (fast_2d_coarse.hip,
PlanFrontEnd), so what holds here holds for the launches.

The fused launch is ONE for all fused problems of a call: three scans of points in LDS as soon
as any problem is grouped, accumulators for the largest problem.  Eligibility is decided per
problem, each with its own accumulators; the sum of the two maxima can exceed what either problem
asked for.  The launch gets 64 KB (the kernel does not opt in to more), so the planner checks the
launch and, where it would not fit, groups nobody.
"""
import numpy as np
import pytest

LDS_LIMIT = 64 * 1024
MISC = 128          # kFusedMisc


def _spec(nx, ny, depth, lin, ang, res=0.05):
    from cartographer_amd import _lib, scan_matching as sm
    return (_lib.Grid2DLimits(res, 10.0, 10.0, nx, ny, sm.K_MIN_CORRESPONDENCE_COST,
                              sm.K_MAX_CORRESPONDENCE_COST), _lib.Fast2DOptions(lin, ang, depth))


def _plan(specs, n, max_range, full=None):
    from cartographer_amd import scan_matching as sm
    return sm.debug_plan(specs, full, num_points=n, max_range_xy=max_range)


def _lds(n, group, acc):
    return 4 * ((n + 63) // 64 * 64) * group + 4 * (MISC + acc) + 1024


def test_worked_example_of_the_lds_overflow():
    """4000 points (n_pad 4032), the farthest 388 cells away, depth 5, windows of 25 m and 0.01
    rad (9 rotations).  A, 60 x 60: 5 x 5 cells per plane, 54 candidates per axis, 62^2
    accumulators, grouped: 12 * 4032 + 4 * (128 + 3844) + 1024 = 65 296 B.  B, 100 x 100: 8 x 8,
    56 per axis, 70^2 accumulators, fused, too large for three scans.  Sized from the two maxima
    their launch asked for 12 * 4032 + 4 * (128 + 4900) + 1024 = 69 520 B and was rejected; the
    planner now checks the launch: nobody grouped, 4 * 4032 + 4 * (128 + 4900) + 1024 = 37 264 B."""
    n, far = 4000, float(np.float32(388 * 0.05))
    A, B = _spec(60, 60, 5, 25.0, 0.01), _spec(100, 100, 5, 25.0, 0.01)
    (a,), la = _plan([A], n, far)
    (b,), lb = _plan([B], n, far)
    assert a == dict(use_planes=1, plane_stride=64, use_fused=1, group=3, num_scans=9, acc=62 * 62)
    assert b == dict(use_planes=1, plane_stride=64, use_fused=1, group=1, num_scans=9, acc=70 * 70)
    assert la["fused_lds"] == _lds(n, 3, a["acc"]) == 65296 <= LDS_LIMIT and la["per_unit"] == 3
    assert lb["fused_lds"] == _lds(n, 1, b["acc"]) == 37264
    assert _lds(n, 3, b["acc"]) == 69520 > LDS_LIMIT          # what B would need to be grouped
    for specs in ([A, B], [B, A], [A, A, B, A]):
        problems, launch = _plan(specs, n, far)
        former = _lds(n, 3, max(q["acc"] for q in problems))  # any grouped x the largest accumulators
        assert former == 69520 > LDS_LIMIT
        assert [q["group"] for q in problems] == [1] * len(specs)
        assert launch["any_group"] == 0 and launch["per_unit"] == 1
        assert launch["fused_acc"] == 70 * 70 and launch["fused_lds"] == 37264 <= LDS_LIMIT


def test_the_fallback_is_taken_only_where_the_launch_does_not_fit():
    """Random batches of small grids, depth 5 and 6, clouds of 300 ... 4096 points: the launch
    always fits; its sizes are the maxima over its problems; and unless "any grouped" times "the
    largest accumulators" exceeds the limit every problem keeps the decision it gets alone."""
    rng = np.random.default_rng(0)
    dropped = kept = 0
    for trial in range(300):
        depth = int(rng.choice([5, 6]))
        n = int(rng.choice([300, 1000, 2500, 3500, 4000, 4096]))
        max_range = float(np.float32(rng.uniform(2.0, 25.0)))
        specs = [_spec(int(rng.integers(1, 140)), int(rng.integers(1, 140)), depth,
                       float(rng.choice([0.5, 3.0, 25.0])), float(rng.choice([0.0, 0.01, 0.1])))
                 for _ in range(int(rng.integers(2, 6)))]
        full = [int(rng.integers(0, 4) == 0) for _ in specs]
        problems, launch = _plan(specs, n, max_range, full)
        alone = [_plan([s], n, max_range, [f])[0][0] for s, f in zip(specs, full)]
        fused = [q for q in problems if q["use_fused"]]
        if not fused:
            assert launch["fused_lds"] == 0
            continue
        group = 3 if launch["any_group"] else 1
        assert launch["fused_acc"] == max(q["acc"] for q in fused)
        assert launch["fused_lds"] == _lds(n, group, launch["fused_acc"]) <= LDS_LIMIT
        assert launch["any_group"] == int(any(q["group"] > 1 for q in problems))
        assert launch["per_unit"] == (3 if all(q["group"] > 1 for q in fused) else 1)
        assert launch["max_scans"] == max(q["num_scans"] for q in problems)
        wanted = any(q["group"] > 1 for q in alone)
        if wanted and _lds(n, 3, launch["fused_acc"]) > LDS_LIMIT:
            dropped += 1
            assert all(q["group"] == 1 for q in problems)
            for q, one in zip(problems, alone):       # nothing but the grouping changes
                assert dict(q, group=0) == dict(one, group=0)
        else:
            kept += 1
            assert problems == alone
    assert dropped >= 5 and kept >= 100               # (both branches were met)


def test_plan_entry_checks_its_arguments():
    from cartographer_amd import _lib
    with pytest.raises(_lib.CmxError):
        _plan([_spec(10, 10, 13, 1.0, 0.1)], 100, 3.0)         # depth beyond kMaxDepth
    with pytest.raises(_lib.CmxError):
        _plan([_spec(10, 10, 5, 1.0, 0.1)], 0, 3.0)            # empty cloud
    try:
        _lib.debug_set(fast2d_unfused=1)                       # the switches apply as to a match
        (q,), launch = _plan([_spec(100, 100, 5, 1.0, 0.1)], 300, 3.0)
        assert (q["use_planes"], q["use_fused"], launch["fused_lds"]) == (1, 0, 0)
    finally:
        _lib.debug_reset()
