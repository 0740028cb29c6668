"""GPU tier: the whole model on DEVELOPED states of three seasons -- the reference Fortran's own state at 00:00 of 1 April,
1 July and 1 October 1982 (tests/golden/season_<mmdd>_*.npz; layout, restart recipe and the perturbed member:
tests/season_cases.py).  Every other comparison of the device model with the reference or the oracle starts from the resting
atmosphere and ends in January, or is statistical (tests/test_long_gpu.py); here 12 steps (four shortwave steps) run on a state
with jets and convection in motion, slab land, sea and ice models that carry months of memory, and the forcing of the season.

An EnsembleModel of two members is initialised at the date and restarted by the recipe: member 0 holds the fixture state,
member 1 the fixture state with t times 1 + 1e-6 N(0, 1), so that a different state sits at a non-zero member offset.  One
`run(12)`.  Each member is compared with an oracle run of its own (bit for bit the reference on these states:
tests/test_seasons_oracle.py), under bounds that come from 4 more oracle runs whose prognostics are moved by one-ulp factors:

  per band (tests/band_norms.py) for vor, t, tr, ps at both time levels: err <= clip(32 nu, 1e-13, 1e-11).  div is held by
    whole field only, and band 31 of t is compared exactly with what the state held before the steps: docstring of
    tests/test_seasons_oracle.py, which also asserts that the oracle alone keeps 32 nu under the caps.
  whole field for the five prognostics and the 17 surface and flux fields: err <= max(32 nu_f, 1e-12); the five zonal forcing
    profiles to 1e-13; the date and the month index equal.

Member 0 is held to the reference's own bits (ref12_*) under the same bounds.  On 1 July a second model stepped as 12 x run(1)
must equal the run(12) model bit for bit in every registry variable (tests/test_run_gpu.py has that equality from rest).

Observed on the MI355X (profiles/seasons_parity.txt), worst over the three dates and both members: per band error / bound
0.146 (1 October, member 0); whole field error 2.6e-13 (1 July), error / bound 0.046.  The figures of a run are printed, and
written to seasons_parity.txt in the directory that the environment variable PYSPEEDY_AMD_REPORT_DIR names, when it is set."""
import os

import numpy as np
import pytest

import band_norms as bn
import season_cases as sc

pytestmark = pytest.mark.gpu

TAGS = list(sc.DATES)
BAND_NAMES = ("vor", "t", "tr", "ps")
REPORT = {}  # tag -> text


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


def device_model(spectral, bc, fix, states):
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, len(states))
    model.set_bc(bc, start_date=tuple(int(v) for v in fix["date"]) + (0, 0))
    sc.restart(model, fix, member=-1)
    for member, state in enumerate(states):
        for name in sc.SPEC:
            model.set(name, state[name], member)
    assert model.current_step == 0
    return model


def compare(tag, what, got, ref, nu, nu_f, t_start):
    """got, ref: name -> array after the steps.  -> (failure texts, worst band error / bound, worst whole-field error, worst
    whole-field error / bound)."""
    failures, worst_band, worst_field, worst_ratio = [], 0.0, 0.0, 0.0
    if not np.array_equal(got["t"][sc.BEYOND], t_start[sc.BEYOND]):
        failures.append("%s %s: the steps changed band 31 of t" % (tag, what))
    for name in BAND_NAMES:
        err = bn.band_errors(sc.without_band31(name, got[name]), sc.without_band31(name, ref[name]))
        rows = bn.worst_bands(err, nu[name])
        worst_band = max(worst_band, rows[0][-3] / rows[0][-1])
        over = ~(err <= bn.bound(nu[name]))
        if over.any():
            failures.append("%s %s, %s: %d of %d bands over the bound; the worst:\n%s" % (
                tag, what, name, int(over.sum()), err.size, bn.describe(rows, bn.trailing_names(name))))
    for name in sc.FIELDS:
        err, limit = float(bn.whole_field(got[name], ref[name])), sc.field_bound(nu_f[name])
        worst_field, worst_ratio = max(worst_field, err), max(worst_ratio, err / limit)
        if not err <= limit:
            failures.append("%s %s, %s: whole-field error %.3e over the bound %.3e" % (tag, what, name, err, limit))
    for name in sc.ZONAL:
        err = float(bn.whole_field(got[name], ref[name]))
        if not err <= 1e-13:
            failures.append("%s %s, %s: error %.3e over 1e-13" % (tag, what, name, err))
    return failures, worst_band, worst_field, worst_ratio


def device_snapshot(model, member):
    out = {n: model.get(n, member) for n in sc.FIELDS}
    for name in sc.ZONAL:
        field = model.get(name, member)
        assert np.all(field == field[:1, :]), name
        out[name] = field[0].copy()
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_twelve_steps_from_the_developed_state(spectral, oracle, bc, golden_dir, tag):
    fix = sc.load(golden_dir, tag)
    cases = [sc.case(oracle, bc, fix, tag, member) for member in (0, 1)]
    states = [sc.member_state(fix, member) for member in (0, 1)]
    for name in BAND_NAMES:  # the condition on the inputs (asserted for every case on the CPU tier as well)
        for member in (0, 1):
            assert bn.cap_excess(cases[member]["nu"][name]) <= bn.CAP, (tag, member, name)
    model = device_model(spectral, bc, fix, states)
    model.run(12)
    assert (model.check(2) == 0).all() and model.current_step == 12
    control = model.control()
    date, month_idx = [int(v) for v in model.current_date], int(control.month_idx)
    got = [device_snapshot(model, member) for member in (0, 1)]
    model.close()
    failures, lines = [], []
    for member in (0, 1):
        ref = cases[member]["ref"]
        assert date == list(ref["cal_ymdhm"]) and month_idx == int(ref["cal_month_idx"]), (date, month_idx)
        f, band, field, ratio = compare(tag, "member %d against its oracle run" % member, got[member], ref, cases[member]["nu"],
                                        cases[member]["nu_f"], states[member]["t"])
        failures += f
        lines.append("%s member %d against the oracle: per band worst error / bound %.3f; whole field worst error %.2e, "
                     "worst error / bound %.3f" % (tag, member, band, field, ratio))
    # member 0 against the reference's own bits
    reference = {n: fix["ref12_" + n] for n in sc.FIELDS + sc.ZONAL}
    assert date == list(fix["ref12_cal_ymdhm"]) and month_idx == int(fix["ref12_cal_month_idx"])
    f, band, field, ratio = compare(tag, "member 0 against the reference", got[0], reference, cases[0]["nu"], cases[0]["nu_f"],
                                    states[0]["t"])
    failures += f
    lines.append("%s member 0 against the reference: per band worst error / bound %.3f; whole field worst error %.2e, "
                 "worst error / bound %.3f" % (tag, band, field, ratio))
    assert np.abs(got[1]["t"] - got[0]["t"]).max() > 1e-9 * np.abs(got[0]["t"]).max()  # the members are different states
    REPORT[tag] = "\n".join(lines)
    print(REPORT[tag])
    assert not failures, "\n".join(failures)


def test_single_step_calls_equal_one_multi_step_call_on_a_developed_state(spectral, bc, golden_dir):
    """12 x run(1) against run(12) from the state of 1 July, both members, every registry variable, bit for bit."""
    fix = sc.load(golden_dir, "0701")
    states = [sc.member_state(fix, member) for member in (0, 1)]
    results = []
    for calls in ((12,), (1,) * 12):
        model = device_model(spectral, bc, fix, states)
        for n in calls:
            model.run(n)
        assert model.current_step == 12
        results.append([{n: model.get(n, member) for n in model.variables()} for member in (0, 1)])
        model.close()
    for member in (0, 1):
        different = [n for n in results[0][member] if not np.array_equal(results[0][member][n], results[1][member][n])]
        assert not different, (member, different)
    assert np.abs(results[0][0]["olr"]).max() > 100.0 and (results[0][0]["precnv"] > 0).sum() > 100
    assert not np.array_equal(results[0][0]["t"], results[0][1]["t"])


def test_zz_report():
    out = os.environ.get("PYSPEEDY_AMD_REPORT_DIR")
    assert set(REPORT) == set(TAGS)
    if out and os.path.isdir(out):
        with open(os.path.join(out, "seasons_parity.txt"), "w") as f:
            f.write("\n".join(REPORT[tag] for tag in TAGS) + "\n")
