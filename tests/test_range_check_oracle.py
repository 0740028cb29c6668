"""CPU tier: the oracle's range check (oracle/orc_dynamics.c: orc_check_diagnostics, diagnostics.f90:16-76) against the
REFERENCE's codes at each of its thresholds (tests/golden/range_check.npz, made by oracle/gen_golden_range.py from the cases of
oracle/range_cases.py): both eddy kinetic energies a relative 1e-9 either side of 500 on every level, the global-mean temperature
at 180 and 320 K exactly and one double outside, a zonal mean far above 500, two conditions on different levels, and a state
that is out of range only in the time level the check does not look at -- in time level 1 as the reference's `check` sees them,
and in time level 2 with the levels exchanged."""
import numpy as np
import pytest
import range_cases as RC


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir + "/range_check.npz")


@pytest.fixture(scope="module")
def base(golden_dir):
    return RC.base(np.load(golden_dir + "/run.npz"))


def test_the_stored_cases_are_the_ones_range_cases_builds(oracle, gold, base):
    rc, diag = RC.oracle_check(oracle, base, 1)
    assert rc == 0
    assert np.array_equal(diag[:, :2], gold["ke_base"])
    names, edits = RC.table(gold["ke_base"])
    assert np.array_equal(names, gold["names"]) and np.array_equal(edits, gold["edits"])
    assert np.array_equal(RC.scales(gold["ke_base"]), gold["ke_scale"]) and float(gold["delta"]) == RC.DELTA
    te = gold["t_edges"]
    assert np.array_equal(te, RC.t_edges())
    assert RC.SQRT_HALF == 0.7071067690849304
    assert RC.SQRT_HALF * te[0] == 320.0 and RC.SQRT_HALF * te[1] > 320.0 and te[1] == np.nextafter(te[0], np.inf)
    assert RC.SQRT_HALF * te[2] == 180.0 and RC.SQRT_HALF * te[3] < 180.0 and te[3] == np.nextafter(te[2], -np.inf)
    # the reference accepts exactly 320 and 180 and everything inside the kinetic-energy edges, and nothing beyond them
    outside = np.array([("above" in n) or ("below_180" in n) or n.endswith("_outside") for n in gold["names"]])
    assert np.array_equal(gold["code"], np.where(outside, -2, 0))
    assert len(gold["names"]) % 8 != 0


@pytest.mark.parametrize("time_level", [1, 2])
def test_oracle_codes_equal_the_reference_at_every_edge(oracle, gold, base, time_level):
    wrong = []
    for i, name in enumerate(gold["names"]):
        state = RC.build(base, gold["edits"], i)
        rc, _ = RC.oracle_check(oracle, state if time_level == 1 else RC.swap(state), time_level)
        if rc != gold["code"][i]:
            wrong.append((str(name), rc))
    assert not wrong, wrong


def test_each_edge_moves_only_its_own_diagnostic_to_the_threshold(oracle, gold, base):
    """A kinetic-energy case sits within 1e-12 (relative) of 500 (1 -+ delta): delta = 1e-9 is far outside the noise of the
    summation order.  A temperature case is exactly 320 / 180 K or the next value outside.  Everything else is the base."""
    _, ref = RC.oracle_check(oracle, base, 1)
    delta, te = float(gold["delta"]), gold["t_edges"]
    for i, name in enumerate(gold["names"]):
        name = str(name)
        if not name[-3:-1] == "_l":
            continue
        level = int(name[-1])
        _, diag = RC.oracle_check(oracle, RC.build(base, gold["edits"], i), 1)
        expect = ref.copy()
        if "_ke_" in name:
            col = 0 if name.startswith("vor") else 1
            target = 500.0 * (1.0 + delta if "above" in name else 1.0 - delta)
            assert abs(diag[level, col] - target) <= 1e-12 * target, (name, diag[level, col])
            expect[level, col] = diag[level, col]
        else:
            expect[level, 2] = RC.SQRT_HALF * te[["t_320", "t_above_320", "t_180", "t_below_180"].index(name[:-3])]
        assert np.array_equal(diag, expect), name
