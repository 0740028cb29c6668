"""GPU tier: the STEPPING model against the CPU oracle on boundary sets other than the example -- `mirrored`, `icy` and `patchy` of
tests/boundary_cases.py, on which the oracle is pinned to the reference bit for bit (tests/test_boundaries_oracle.py) and meets,
alone, the conditions the bounds below rest on (tests/test_boundary_cases_cpu.py).  What a step runs downstream of the boundary
fields -- coupler_point.hpp, forcing_kernel's albedo and snow cover, the land / sea weighting of the surface fluxes, the fresh /
re-use schedule of the day's interpolated climatologies -- has otherwise only ever seen one mask, one ice edge, one snow cover and
one orography, the same in every member of every launch.

a. Four planets in ONE launch (example, mirrored, icy, patchy as members 0-3, members 1-3 with a temperature perturbation), 12 steps
   as one call from 1 January 00:00 and from 30 June 20:00 (midnight and a month boundary inside the call), every member against an
   oracle run of its own: whole fields to 1e-11 of the field's maximum (the oracle's own one-ulp sensitivity on these sets is at
   most 1.4e-13), t, tr and ps per level, time level and total wavenumber to clip(32 nu, 1e-13, 1e-11) (tests/band_norms.py),
   band 31 of t untouched by the steps, the calendar, the range check.
b. The same members in every form the step has, bit for bit.  The coupling of a STEP always rides as tail blocks of
   spectral_step_kernel (model.hip, issue_group -> step_range -> run_spectral_step with CouplerArgs; dynamics.hip:545-551); the
   stand-alone coupler_kernel (surface.hip) runs only inside `init` (couple(m, 0, s), day 0), for every member count -- so both
   forms of coupler_point are in every model below, and no member count moves a step's coupling into coupler_kernel.  The forms of
   the step kernel the sizes hit (dynamics.hip:531-539, model.hip:1049):
     1 and 4 members   one group; geopotential folded in (<= 8 members), loads up front (EARLY: launches of <= 8 members)
     24 members, default plan   3 member groups of 8 on streams of their own (model.hip:596), no fold, EARLY, the rim detected on
                       the call's first step and skipped afterwards (model.hip:1499), longwave transmissivities recomputed
                       (kTauFromMembers = 20 <= the round's 24); each group's tail blocks cover members first ... first + 7
     24 members, member_groups 2 and block_members 1   12 rounds of 2 groups of ONE member (step_plan.hpp:26-34): `first` = 0 ... 23,
                       transmissivities from rad_tau2 (rounds of 2 < 20)
     24 members, member_groups 2   2 groups of 12: the form that loads where the values are needed (launches of > 8 members), which
                       neither size above reaches; added for that reason
   and twelve one-step calls (one group, every step stores all diagnostics, no rim detection) against one call of twelve.
c. A host that writes between two calls of one day: only the model's own dirty flag can make the next coupling interpolate again.
   The oracle interpolates at every step, so the device must agree with it after the write as before: the fields of (a) to
   1e-11, the call bit for bit equal to a device run that interpolates at every step, and snow_depth, soil_avail_water, sice_am and
   sstan_am -- copies of interpolated climatologies -- bit for bit equal to the ORACLE.  The last demand found `forint` fused
   into one multiply-add on the device, one ulp from the reference; it rounds twice now (profiles/boundary_parity.txt).

Sensitivity (profiles/boundary_parity.txt): without the 0.5 clamp of coupler_point.hpp, with one `surf_cache_valid = false` taken
out of spd_model_set, or with member 0's climatologies read for every member, (a), (b) or (c) fail."""
import os

import numpy as np
import pytest

import band_norms as bn
import boundary_cases as bcs
from test_model_vs_oracle_gpu import check_bands

pytestmark = pytest.mark.gpu

PLANETS = ("example",) + bcs.SETS  # member i of the four-planet model; member i of a larger one carries PLANETS[i % 4]
TOL = 1e-11


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(os.path.join(golden_dir, "..", "..", "pyspeedy_amd", "data", "example_bc.npz"))


def planets(spectral, bc, start, members, options=()):
    """An EnsembleModel whose member i runs on the set PLANETS[i % 4], initialised at `start`, the temperature of every member
    that is not on the example multiplied by its set's perturbation.  -> (model, the temperature of every member before the first step)"""
    from pyspeedy_amd.model import EnsembleModel
    ens = EnsembleModel(spectral, members)
    for i in range(members):
        bcs.set_member(ens, bcs.fields(bc, PLANETS[i % 4]), i)
    ens.init_sst_anom(bcs.N_MONTHS)
    ens.init(start)
    for name, value in options:
        ens.set_option(name, value)
    t_start = []
    for i in range(members):
        t = ens.get("t", i)
        if i % 4:
            t = t * bcs.perturbation(bcs.MEMBER[PLANETS[i % 4]])
            ens.set("t", t, i)
        t_start.append(t)
    return ens, t_start


def one_planet(spectral, bc, start, k):
    """Member k of the four-planet model as a model of one member."""
    from pyspeedy_amd.model import EnsembleModel
    single = EnsembleModel(spectral, 1)
    bcs.set_member(single, bcs.fields(bc, PLANETS[k]), -1)
    single.init_sst_anom(bcs.N_MONTHS)
    single.init(start)
    if k:
        single.set("t", single.get("t", 0) * bcs.perturbation(bcs.MEMBER[PLANETS[k]]))
    return single


def snapshot(model, member, names):
    return {n: bcs.get(model, n, member) for n in names}


def worst_whole_field(got, ref, names, where, report):
    worst = 0.0
    for n in names:
        scale = np.abs(ref[n]).max()
        err = float(np.abs(got[n].reshape(ref[n].shape) - ref[n]).max() / (scale if scale > 0 else 1.0))
        report.append("%s %s: %.2e" % (where, n, err))
        assert err <= TOL, report[-1]
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize("start", bcs.START_DATES, ids=bcs.tag)
def test_four_planets_in_one_launch_against_an_oracle_run_each(spectral, oracle, bc, start):
    ens, t_start = planets(spectral, bc, start, 4)
    ens.run(12)
    assert (ens.check(2) == 0).all()
    report, band_failures, worst, worst_band = [], [], 0.0, 0.0
    for k, name in enumerate(PLANETS):
        c = bcs.case(oracle, bc, name, start)
        assert not any(c["codes"])
        got = snapshot(ens, k, bcs.FIELDS)
        where = "%s %s" % (name, bcs.tag(start))
        worst = max(worst, worst_whole_field(got, c["ref"], bcs.FIELDS, where, report))
        failed, ratio = check_bands(k, 12, bcs.BAND_NAMES, got, bcs.Held(c["ref"]), c["noisy"], (t_start[k].reshape(31, 32, 8, 2), c["t_start"]))
        report.append("%s per band: worst error / bound %.3f" % (where, ratio))
        band_failures += failed
        worst_band = max(worst_band, ratio)
        assert (list(ens.current_date), ens.control().month_idx) == c["calendar"], (ens.current_date, c["calendar"])
    # (the four members are four different planets, not one)
    assert not np.array_equal(ens.get("sice_am", 0), ens.get("sice_am", 1)) and not np.array_equal(ens.get("fmask_land", 0), ens.get("fmask_land", 3))
    print("\n".join(report))
    print("four planets x 12 steps from %s against the oracle: worst scaled error %.2e; per band: worst error / bound %.3f" % (
        bcs.tag(start), worst, worst_band))
    assert not band_failures, "\n".join(band_failures)
    ens.close()


@pytest.mark.parametrize("start", bcs.START_DATES, ids=bcs.tag)
def test_the_same_planets_in_every_form_of_the_step_are_bitwise(spectral, bc, start):
    names = bcs.EXACT_FORMS
    four, _ = planets(spectral, bc, start, 4)
    four.run(12)
    ref = [snapshot(four, k, names) for k in range(4)]
    four.close()
    assert np.abs(ref[2]["rad_tau2"]).max() > 0 and np.abs(ref[3]["olr"]).max() > 100.0

    def same(model, member, k, form):
        for n in names:
            assert np.array_equal(bcs.get(model, n, member), ref[k][n]), (form, member, n)

    for k in range(4):
        single = one_planet(spectral, bc, start, k)
        single.run(12)
        same(single, 0, k, "one member")
        single.close()
    stepwise, _ = planets(spectral, bc, start, 4)
    for _ in range(12):
        stepwise.run(1)
    for k in range(4):
        same(stepwise, k, k, "twelve one-step calls")
    stepwise.close()
    for form, options, chunks, rounds in (("24 members, default plan", (), 3, 1),
                                          ("24 members in rounds", (("member_groups", 2), ("block_members", 1)), 2, 12),
                                          ("24 members in two groups of 12", (("member_groups", 2),), 2, 1)):
        large, _ = planets(spectral, bc, start, 24, options)
        cfg = large.config()
        assert (cfg["chunks"], cfg["rounds"], cfg["fold_geo"]) == (chunks, rounds, False), (form, cfg)
        large.run(12)
        assert (large.check(2) == 0).all()
        for i in range(24):
            same(large, i, i % 4, form)
        large.close()


# name of the case -> (the field the write drives, the registry array written and what becomes of its value; None: a flag)
HOST_WRITES = {
    "sst12": ("sst_am", "sst12", lambda v: v + 0.5),
    "sea_ice_frac12": ("sice_am", "sea_ice_frac12", lambda v: 0.5 * v),
    "snowd12": ("snow_depth", "snowd12", lambda v: 2 * v),
    "stl12": ("land_temp", "stl12", lambda v: v - 1),
    "soilw12": ("soil_avail_water", "soilw12", lambda v: 0.5 * v),
    "sst_anom": ("sstan_am", "sst_anom", lambda v: bcs.anomaly()),  # (the anomaly flag is on, as by default; zero planes until here)
    "land_coupling_off": ("land_temp", None, None),
}
EXACT_AFTER_A_WRITE = ("snow_depth", "soil_avail_water", "sice_am", "sstan_am")
_plain = {}


def oracle_without_the_write(oracle, bc):
    """FIELDS of the oracle on `icy` after 12 undisturbed steps from 1 January 00:00; computed once, read-only."""
    if not _plain:
        m = bcs.oracle_model(oracle, bcs.fields(bc, "icy"), bcs.START_DATES[0])
        assert all(m.step() == 0 for _ in range(12))
        _plain.update({n: bcs.get(m, n) for n in bcs.FIELDS})
    return _plain


_written = {}


def written_run(spectral, oracle, bc, write):
    """5 steps from 1982-01-01 00:00 on `icy`, the write `write` on both sides, 7 more steps, all before midnight.
    -> (device, oracle: fields after the 12 steps, the field the write drives, a second device model whose 7 steps after the write
    are one-step calls behind `invalidate()`); run once per session and write, read-only."""
    if write in _written:
        return _written[write]
    from pyspeedy_amd.model import EnsembleModel
    start = bcs.START_DATES[0]
    b = bcs.fields(bc, "icy")
    cpu = bcs.oracle_model(oracle, b, start)
    gpu, always_fresh = EnsembleModel(spectral, 1), EnsembleModel(spectral, 1)
    for m in (gpu, always_fresh):
        bcs.set_member(m, b, -1)
        m.init_sst_anom(bcs.N_MONTHS)
        m.init(start)
        m.run(5)
    assert all(cpu.step() == 0 for _ in range(5))
    driven, name, change = HOST_WRITES[write]
    if name is None:
        for m in (gpu, always_fresh):
            m.set_flags(land_coupling_flag=False)
        cpu.set("land_coupling_flag", 0)
    else:
        value = change(cpu.get(name))
        for m in (gpu, always_fresh, cpu):
            m.set(name, value)
    gpu.run(7)
    for _ in range(7):  # every coupling interpolates, as the oracle's does
        always_fresh.invalidate()
        always_fresh.run(1)
    assert all(cpu.step() == 0 for _ in range(7))
    assert gpu.current_date == always_fresh.current_date == (1982, 1, 1, 8, 0) and (gpu.check(2) == 0).all()
    _written[write] = (snapshot(gpu, 0, bcs.EXACT_FORMS), {n: bcs.get(cpu, n) for n in bcs.FIELDS}, driven,
                       snapshot(always_fresh, 0, bcs.EXACT_FORMS))
    gpu.close()
    always_fresh.close()
    return _written[write]


@pytest.mark.parametrize("write", list(HOST_WRITES))
def test_a_host_write_between_two_calls_of_one_day_reaches_the_next_coupling(spectral, oracle, bc, write):
    """The device against the oracle, which interpolates the climatologies at every step: the whole fields of (a) to 1e-11.  A
    coupling that re-used the day's stored climatologies after the write would miss by the size of the write (asserted to be more
    than 1e-6 of the driven field's maximum in the oracle)."""
    got, ref, driven, _ = written_run(spectral, oracle, bc, write)
    # the case proves something only if the write matters to the oracle
    moved = bn.whole_field(oracle_without_the_write(oracle, bc)[driven], ref[driven])  # (of the maximum of the field WITH the write)
    assert moved > 1e-6, (write, driven, moved)
    report = []
    worst = worst_whole_field(got, ref, bcs.FIELDS, write, report)
    print("\n".join(report))
    print("write %s: the oracle's %s moved by %.2e; device against oracle, worst scaled error %.2e" % (write, driven, moved, worst))


@pytest.mark.parametrize("write", list(HOST_WRITES))
def test_after_a_host_write_the_call_equals_a_device_run_that_interpolates_at_every_step(spectral, oracle, bc, write):
    """Exactness the device owes whatever its rounding: the 7 steps after the write as ONE call, whose couplings re-use what the
    first one stored, against seven one-step calls each behind `invalidate()`, whose couplings all interpolate -- every name of (b),
    bit for bit."""
    got, _, driven, fresh = written_run(spectral, oracle, bc, write)
    for n in bcs.EXACT_FORMS:
        assert np.array_equal(got[n], fresh[n]), (write, n)


@pytest.mark.parametrize("write", list(HOST_WRITES))
def test_what_a_fresh_coupling_copies_from_the_climatologies_equals_the_oracle_exactly(spectral, oracle, bc, write):
    """snow_depth, soil_avail_water, sice_am and sstan_am after the write and 7 more steps, bit for bit against the oracle.

    These are copies of what `forint` and the anomaly interpolation return (coupler_point.hpp), so they owe the reference's bits.
    This test found that they did not have them, write or no write: the interpolation a + w * (b - a) was one expression, which
    device code (-ffp-contract=on) fuses into one multiply-add, while interpolation.f90 rounds twice -- soil_avail_water off by one
    ulp at 72 points (on the example planet too, and right after `init`), sice_am at 28 (1 on the example), sstan_am at 806 once
    the anomaly planes are written; snow_depth exact only because snowd12 holds single-precision values.  The product and the sum
    are two statements now (profiles/boundary_parity.txt, section 3)."""
    got, ref, _, _ = written_run(spectral, oracle, bc, write)
    different = []
    for n in EXACT_AFTER_A_WRITE:
        d = got[n] != ref[n]
        if d.any():
            different.append("%s: %d points, at most %.1f ulp" % (n, d.sum(), (np.abs(got[n][d] - ref[n][d]) / np.spacing(np.abs(ref[n][d]))).max()))
    print("write %s: %s" % (write, "; ".join(different) or "all four exact"))
    assert not different, (write, different)
