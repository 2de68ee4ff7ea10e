"""The case table of tests/ceres_edge_cases.py on the oracle alone, so that the device tests of
tests/test_gpu_ceres_edges.py cannot pass vacuously:

  * every case reaches what it is named for (termination code, rejected steps, points outside
    the grid and stencils across the named edge or face, at least one step on the tiny clouds);
  * every case is stable: the oracle's step counts and termination do not change when the cloud
    is reordered (20 random orders: another order of the f64 sums) or the initial angle moves by
    one ulp (sin / cos an ulp apart) -- the two legitimate differences of the device.  A case
    whose counts change sits on an accept / reject threshold and is replaced, not loosened: no
    case is excluded on the device side;
  * the one-step tolerance, 1000 x the largest pose change those perturbations cause over the
    one_step cases, comes out at or below 1e-10;
  * where the reference's own cost functions are built (oracle/_ref), the one_step and border
    inputs give the same pose (1e-9) and counts there as on the restatement.
"""
import numpy as np
import pytest

import ceres_edge_cases as ec


NAMES_2D, NAMES_3D = ec.NAMES_2D, ec.NAMES_3D


@pytest.fixture(scope="module")
def table_2d(synth):
    return {c.name: c for c in ec.cases_2d(synth)}


@pytest.fixture(scope="module")
def table_3d(synth, oracle):
    return {c.name: c for c in ec.cases_3d(synth, oracle)}


def _check_expectations(case, result, outside, straddling):
    print(case.name, ec.counts(result), "cost %.6g -> %.6g" % (result["initial_cost"],
                                                              result["final_cost"]),
          "outside", outside, "straddling", straddling)
    if case.termination is not None:
        assert result["termination"] == case.termination
    if case.steps is not None:
        assert ec.counts(result)[:2] == case.steps
    assert result["num_successful_steps"] >= case.min_successful
    assert result["num_unsuccessful_steps"] >= case.min_unsuccessful
    assert outside >= case.min_outside
    for edge, least in case.min_straddling.items():
        assert straddling[edge] >= least, (edge, straddling)


def _check_stable(result, perturbed):
    changed = [ec.counts(p) for p in perturbed if ec.counts(p) != ec.counts(result)]
    assert not changed, (ec.counts(result), changed)
    spread = max(float(np.abs(p["pose"] - result["pose"]).max()) for p in perturbed)
    print("pose spread under reordering and +-1 ulp of the angle: %.3g" % spread)
    assert spread < 1e-9           # far inside the whole-solve bar of 1e-6


def test_the_table_holds_every_family_and_size():
    for names in (NAMES_2D, NAMES_3D):
        assert len(set(names)) == len(names)
        for family in ("one_step", "border", "step", "size"):
            assert any(n.startswith(family) for n in names), family
        for n in ec.SIZES:
            assert "size_%d" % n in names
    assert {"size_1_and_1000", "size_1000_and_1", "border_negative_indices",
            "border_all_outside"} <= set(NAMES_3D)


@pytest.mark.parametrize("name", NAMES_2D)
def test_2d_case_reaches_its_branch_and_is_stable(synth, oracle, table_2d, name):
    case = table_2d[name]
    sc = ec.scene_2d(synth)
    assert (sc.lim["num_x_cells"], sc.lim["num_y_cells"]) == (ec.NX_2D, ec.NY_2D) and \
        ec.NX_2D != ec.NY_2D
    assert case.cloud.shape[0] == (int(name[5:]) if case.family == "size" else 300)
    result = ec.oracle_2d(oracle, synth, case)
    outside, straddling = ec.stencils_2d(sc.lim, case.init, case.cloud)
    _check_expectations(case, result, outside, straddling)
    if name == "border_all_outside_zero_gradient":
        np.testing.assert_array_equal(result["pose"], case.init)
    _check_stable(result, ec.perturbed_2d(oracle, synth, case))


@pytest.mark.parametrize("name", NAMES_3D)
def test_3d_case_reaches_its_branch_and_is_stable(synth, oracle, table_3d, name):
    case = table_3d[name]
    result = ec.oracle_3d(oracle, case)
    first = case.pairs[0]
    outside, straddling, corrected = ec.gathers_3d(first[1], first[2], case.init7(), first[0])
    _check_expectations(case, result, outside, straddling)
    if case.family == "border" and name != "border_all_outside":
        # both sides of `if (centre > point) centre -= resolution`
        assert 0 < corrected < 3 * first[0].shape[0]
    if name == "border_all_outside":
        np.testing.assert_allclose(result["pose"], case.init7(), rtol=0, atol=1e-15)
    if name == "border_negative_indices":
        assert all(p[2][a].max() < 0 for p in case.pairs for a in "xyz")
    _check_stable(result, ec.perturbed_3d(oracle, case))


def test_rejected_steps_make_the_nonmonotonic_solves_differ(synth, oracle, table_2d, table_3d):
    """The non-monotonic bookkeeping is exercised: with rejected steps on both sides the two
    step rules walk different iterates."""
    for table, run in ((table_2d, lambda c: ec.oracle_2d(oracle, synth, c)),
                       (table_3d, lambda c: ec.oracle_3d(oracle, c))):
        pairs = [(n, n.replace("_monotonic", "_nonmonotonic")) for n in table
                 if n.startswith("step_") and n.endswith("_monotonic")]
        assert len(pairs) >= 2
        for plain, nonmono in pairs:
            assert ec.counts(run(table[plain])) != ec.counts(run(table[nonmono])), plain
    capped = [n for n in NAMES_3D if n.startswith("step_") and
              ec.oracle_3d(oracle, table_3d[n])["termination"] == ec.TERMINATION_NO_CONVERGENCE]
    assert len(capped) >= 2, capped


def test_one_step_tolerance_is_measured_and_small(synth, oracle):
    spread_2d, spread_3d = ec.one_step_spread(oracle, synth)
    tolerance = ec.one_step_tolerance(oracle, synth)
    print("one-step pose spread: 2D %.3g, 3D %.3g; tolerance %.3g" % (spread_2d, spread_3d,
                                                                      tolerance))
    assert spread_2d > 0.0 and spread_3d > 0.0
    assert tolerance == ec.ONE_STEP_FACTOR * max(spread_2d, spread_3d) <= ec.ONE_STEP_CEILING
    # the steps the tolerance is held against are eight and more orders larger
    for case in ec.cases_2d(synth):
        if case.family == "one_step":
            step = np.abs(ec.oracle_2d(oracle, synth, case)["pose"] - np.array(case.init)).max()
            assert step > 1e-2, (case.name, step)
    for case in ec.cases_3d(synth, oracle):
        if case.family == "one_step":
            step = np.abs(ec.oracle_3d(oracle, case)["pose"] - np.array(case.init7())).max()
            assert step > 5e-3, (case.name, step)


# ------------------------------------------------ the reference's own cost functions ------------
@pytest.fixture(scope="module")
def refc(oracle):
    lib = oracle.ref_ceres_lib()
    if lib is None:
        pytest.skip("reference tree not available and oracle/_ref/libref_ceres.so not prebuilt")
    return lib


def _same_as_the_reference(a, b):
    """The bar of tests/test_reference_ref_ceres.py."""
    np.testing.assert_allclose(a["pose"], b["pose"], rtol=0, atol=1e-9)
    assert a["initial_cost"] == pytest.approx(b["initial_cost"], rel=1e-12)
    assert a["final_cost"] == pytest.approx(b["final_cost"], rel=1e-9)
    assert ec.counts(a) == ec.counts(b)


@pytest.mark.parametrize("name", [n for n in NAMES_2D if n.startswith(("one_step", "border"))])
def test_2d_case_on_the_reference_cost_functions(refc, synth, oracle, table_2d, name):
    case = table_2d[name]
    _same_as_the_reference(ec.oracle_2d(oracle, synth, case),
                           ec.oracle_2d(oracle, synth, case, reference=True))


@pytest.mark.parametrize("name", [n for n in NAMES_3D if n.startswith(("one_step", "border"))])
def test_3d_case_on_the_reference_cost_functions(refc, oracle, table_3d, name):
    case = table_3d[name]
    _same_as_the_reference(ec.oracle_3d(oracle, case), ec.oracle_3d(oracle, case, reference=True))
