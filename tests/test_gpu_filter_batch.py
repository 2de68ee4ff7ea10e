"""cmx_filter_batch on the device: every job of a call -- on a host cloud or chained on an earlier
job's output -- returns the counts, indices and points of the single calls on the same input, and
of the oracle where it takes the input."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def filters():
    from cartographer_amd import _lib, filters
    assert _lib.lib().cmx_device_count() >= 1, "no HIP device: these tests need the GPU"
    return filters


def _normal(seed, n, sigma=3.0, flat=False):
    """A normal cloud with exact duplicates (the values alone cannot tell which point was kept)."""
    rng = np.random.default_rng(seed)
    cloud = rng.normal(0.0, sigma, (n, 3))
    if flat:
        cloud = cloud * np.array([1.0, 1.0, 0.2])
    cloud = cloud.astype(np.float32)
    k = len(cloud[1::7])
    cloud[::7][:k] = cloud[1::7]
    return cloud


def _scan(seed, n):
    """A planar range scan: a ring of returns between 2 and 20 m, some rays hitting twice."""
    rng = np.random.default_rng(seed)
    angle = np.sort(rng.uniform(-np.pi, np.pi, n))
    r = 8.0 + 6.0 * np.sin(3.0 * angle) + rng.normal(0.0, 0.02, n)
    cloud = np.stack([r * np.cos(angle), r * np.sin(angle), np.zeros(n)], 1).astype(np.float32)
    cloud[::11][:len(cloud[1::11])] = cloud[1::11]
    return cloud


def voxel(length, **more):
    return dict(mode="voxel", length=length, **more)


def adaptive(max_length, min_num_points, max_range, **more):
    return dict(mode="adaptive", length=max_length, min_num_points=min_num_points,
                max_range=max_range, **more)


def _single(filters, job, xyz):
    if job["mode"] == "voxel":
        return (filters.voxel_filter_indices(xyz, job["length"]),
                filters.voxel_filter(xyz, job["length"]))
    args = (job["length"], job["min_num_points"], job["max_range"])
    return (filters.adaptive_voxel_filter_indices(xyz, *args),
            filters.adaptive_voxel_filter(xyz, *args))


def check(filters, oracle, jobs, got=None):
    """Runs `jobs` in one call and compares every job with the single calls on the same input -- a
    chained job's input being the points the batch (or, for a parent without outputs, the single
    call) returned for its parent -- and with the oracle."""
    if got is None:
        got = filters.filter_batch(jobs)
    assert len(got) == len(jobs)
    inputs = {}
    for k, job in enumerate(jobs):
        if job.get("input_job", -1) < 0:
            xyz = np.ascontiguousarray(job["cloud"], np.float32).reshape(-1, 3)
        else:
            xyz = inputs[job["input_job"]]
        indices, points = _single(filters, job, xyz)
        inputs[k] = got[k]["points"] if got[k]["points"] is not None else points
        if job.get("indices", True):
            np.testing.assert_array_equal(got[k]["indices"], indices, err_msg=f"job {k}")
        else:
            assert got[k]["indices"] is None
        if job.get("points", True):
            np.testing.assert_array_equal(got[k]["points"], points, err_msg=f"job {k}")
            np.testing.assert_array_equal(points, xyz[indices], err_msg=f"job {k}")
        else:
            assert got[k]["points"] is None
        if len(xyz) == 0:
            assert len(indices) == 0            # (for empty inputs the single call is the yardstick)
            continue
        if job["mode"] == "voxel":
            want = np.nonzero(oracle.voxel_filter_flags(xyz, job["length"]))[0]
            np.testing.assert_array_equal(indices, want, err_msg=f"job {k}")
        else:
            want = oracle.adaptive_voxel_filter(xyz, job["length"], job["min_num_points"],
                                                job["max_range"])
            np.testing.assert_array_equal(points, want, err_msg=f"job {k}")
    return got


SIZES = (1, 63, 64, 65, 1000, 2048, 2049, 4096)


def test_one_call_with_mixed_sizes_in_both_modes(filters, oracle):
    jobs = []
    for seed, n in enumerate(SIZES):
        cloud = _normal(seed, n)
        jobs += [voxel(0.3, cloud=cloud), adaptive(0.5, 200, 50.0, cloud=_normal(20 + seed, n))]
    plans, call = filters.filter_batch_plan(jobs)
    assert call["num_launches"] == 2 and not any(p["single"] for p in plans)
    got = check(filters, oracle, jobs)
    assert len(got[0]["indices"]) == 1 and len(got[1]["indices"]) == 1       # n = 1


def test_voxel_edge_cases(filters, oracle):
    same = np.tile(np.array([[-100.0, 0.3, 0.4]], np.float32), (100, 1))
    rng = np.random.default_rng(10)
    apart = rng.normal(0.0, 3.0, (4000, 3)).astype(np.float32)
    got = check(filters, oracle, [voxel(0.3, cloud=same), voxel(1e-4, cloud=apart),
                                  voxel(1000.0, cloud=apart)])
    assert len(got[0]["indices"]) == 1
    assert len(got[1]["indices"]) == 4000          # every voxel has its own point
    assert len(got[2]["indices"]) == 1             # all points in one voxel: 3999 draws


def test_adaptive_edge_cases(filters, oracle):
    few = _normal(3, 100, 8.0, flat=True)                        # n <= min_num_points
    far = _normal(9, 2500, 8.0, flat=True)                       # max_range removes every point
    rng = np.random.default_rng(4)                               # the bisection down to small voxels
    dense = (rng.normal(0.0, 8.0, (3000, 3)) * np.array([1.0, 1.0, 0.2])).astype(np.float32)
    got = check(filters, oracle, [adaptive(0.5, 200, 50.0, cloud=few),
                                  adaptive(0.5, 200, 0.01, cloud=far),
                                  adaptive(0.9, 2900, 80.0, cloud=dense),
                                  adaptive(0.5, 100, 50.0, cloud=few)])     # n == min_num_points
    in_range = np.nonzero(np.linalg.norm(few.astype(np.float64), axis=1) <= 50.0)[0]
    assert len(in_range) == 100
    np.testing.assert_array_equal(got[0]["indices"], in_range)   # the in-range cloud unfiltered
    np.testing.assert_array_equal(got[3]["indices"], in_range)
    assert len(got[1]["indices"]) == 0 and got[1]["points"].shape == (0, 3)
    assert 2900 <= len(got[2]["indices"]) < 3000


def test_the_chain_of_the_2d_builder(filters, oracle):
    scan = _scan(1, 1000)
    jobs = [voxel(0.025, cloud=scan), adaptive(0.5, 200, 50.0, input_job=0)]
    plans, call = filters.filter_batch_plan(jobs)
    assert [(p["stage"], p["N"]) for p in plans] == [(0, 1024), (1, 1024)]
    assert call["num_launches"] == 2
    got = check(filters, oracle, jobs)
    assert 200 <= len(got[1]["indices"]) < len(got[0]["indices"]) < 1000
    # the child's indices refer to the parent's output: composed, they select from the scan
    through = got[0]["indices"][got[1]["indices"]]
    np.testing.assert_array_equal(scan[through], got[1]["points"])


def test_the_chain_of_the_3d_builder(filters, oracle):
    cloud = _normal(2, 4000, 8.0, flat=True)
    jobs = [voxel(0.15, cloud=cloud), adaptive(2.0, 150, 15.0, input_job=0),
            adaptive(4.0, 200, 60.0, input_job=0)]
    got = check(filters, oracle, jobs)
    assert len(got[1]["indices"]) >= 150 and len(got[2]["indices"]) >= 200
    assert len(got[1]["indices"]) != len(got[2]["indices"])


def test_chains_on_an_empty_parent_and_on_a_parent_without_outputs(filters, oracle):
    scan = _scan(2, 700)
    jobs = [voxel(0.1, cloud=np.zeros((0, 3), np.float32)),
            adaptive(0.5, 200, 50.0, input_job=0),
            voxel(0.05, cloud=scan, indices=False, points=False),
            adaptive(0.5, 200, 50.0, input_job=2),
            voxel(0.5, input_job=2, points=False),
            adaptive(0.5, 200, 0.01, cloud=scan),         # a parent that keeps nothing
            voxel(0.1, input_job=5)]
    got = check(filters, oracle, jobs)
    assert len(got[0]["indices"]) == 0 and len(got[1]["indices"]) == 0
    assert got[2] == dict(indices=None, points=None)
    assert len(got[3]["indices"]) >= 200 and len(got[4]["indices"]) > 0
    assert len(got[5]["indices"]) == 0 and len(got[6]["indices"]) == 0


def test_a_parent_of_4096_points_whose_child_keeps_all_of_them(filters, oracle):
    rng = np.random.default_rng(12)
    cloud = rng.normal(0.0, 3.0, (4096, 3)).astype(np.float32)
    jobs = [voxel(1e-4, cloud=cloud), adaptive(0.5, 200, 50.0, input_job=0),
            voxel(1e-4, input_job=0)]
    plans, _ = filters.filter_batch_plan(jobs)
    assert [(p["N"], p["launch"]) for p in plans] == [(4096, 1)] * 3
    got = check(filters, oracle, jobs)
    assert len(got[0]["indices"]) == 4096 and len(got[2]["indices"]) == 4096


def test_two_jobs_share_one_input(filters, oracle):
    cloud = _normal(5, 1500, 8.0, flat=True)
    jobs = [voxel(0.3, cloud=cloud), adaptive(0.5, 200, 50.0, cloud=cloud),
            voxel(0.3, cloud=cloud.copy())]
    plans, call = filters.filter_batch_plan(jobs)
    assert [p["cloud_slot"] for p in plans] == [0, 0, 1] and call["staged_bytes"] == 2 * 18000
    got = check(filters, oracle, jobs)
    np.testing.assert_array_equal(got[0]["indices"], got[2]["indices"])
    assert len(got[0]["indices"]) != len(got[1]["indices"])


def test_a_large_root_with_a_child_among_small_jobs(filters, oracle):
    small = [voxel(0.3, cloud=_normal(30, 500)), adaptive(0.5, 200, 50.0, cloud=_normal(31, 900)),
             voxel(0.2, cloud=_normal(32, 3000))]
    alone = filters.filter_batch(small)
    large = _normal(33, 5000, 8.0, flat=True)
    jobs = [small[0], voxel(0.15, cloud=large), small[1], adaptive(2.0, 150, 15.0, input_job=1),
            small[2], voxel(0.5, input_job=1, indices=False),
            voxel(0.15, cloud=large, indices=False, points=False), voxel(1.0, input_job=6)]
    plans, _ = filters.filter_batch_plan(jobs)
    assert [p["single"] for p in plans] == [0, 1, 0, 1, 0, 1, 1, 1]
    got = check(filters, oracle, jobs)
    assert len(got[1]["indices"]) > 4096 // 2
    for k, a in zip((0, 2, 4), alone):                       # the other jobs are unaffected
        np.testing.assert_array_equal(got[k]["indices"], a["indices"])
        np.testing.assert_array_equal(got[k]["points"], a["points"])


def test_more_jobs_than_compute_units(filters, oracle):
    jobs = [voxel(0.5, cloud=_normal(100 + k, 300)) if k % 2 else
            adaptive(1.0, 100, 50.0, cloud=_normal(100 + k, 300)) for k in range(600)]
    plans, call = filters.filter_batch_plan(jobs)
    assert call["num_launches"] == 1 and {p["N"] for p in plans} == {512}
    got = check(filters, oracle, jobs)
    assert len({len(g["indices"]) for g in got}) > 10        # distinct seeds, distinct results


def test_a_call_cut_into_sets_returns_the_same(filters, oracle, debug):
    jobs = []
    for r in range(5):
        jobs.append(voxel(0.05, cloud=_scan(40 + r, 1000), points=bool(r % 2)))
    for r in range(5):
        jobs.append(adaptive(0.5, 200, 50.0, input_job=r))
    whole = filters.filter_batch(jobs)
    debug(filter_batch_set_kb=40)
    plans, call = filters.filter_batch_plan(jobs)
    assert call["num_sets"] >= 2 and all(plans[r]["set"] == plans[5 + r]["set"] for r in range(5))
    cut = check(filters, oracle, jobs)
    for a, b in zip(whole, cut):
        for name in ("indices", "points"):
            if a[name] is None:
                assert b[name] is None
            else:
                np.testing.assert_array_equal(a[name], b[name])
