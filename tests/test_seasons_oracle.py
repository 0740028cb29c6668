"""CPU tier: the oracle as a whole model on DEVELOPED states -- the reference Fortran's own state at 00:00 of 1 April, 1 July
and 1 October 1982 of an unperturbed run from 1 January (tests/golden/season_<mmdd>_*.npz, oracle/gen_golden_seasons.py; layout
and restart recipe: tests/season_cases.py).  Everything else that compares the whole model with the reference starts from the
resting atmosphere and ends in January (tests/test_model_oracle.py); here the jets and the convection are in motion, the slab
land, sea and ice models carry months of memory, and the climatology interpolation, the zenith and the ozone forcing are those
of spring, summer and autumn.

1. Oracle against reference, exact bits: an oracle.Model restarted by the recipe equals the reference 12 and 36 steps later in
   all 22 stored fields, the five zonal forcing profiles and the calendar.  That also proves the list of 19 restart arrays
   complete for the oracle (the generator proves it for the reference).
2. The fixtures are what they claim (assertions on the data, observed figures beside them).
3. The conditions under which tests/test_seasons_gpu.py may hold the device to the oracle's own rounding sensitivity, for the
   fixture state (member 0) and the perturbed member 1, NOISE_DRAWS = 4 oracle runs each whose five prognostics are moved by
   one-ulp factors after the restart, 12 steps:
     per band (tests/band_norms.py, MARGIN 32, CAP 1e-11)  32 nu <= 1e-11 for vor, t, tr, ps.  Observed, worst of the three
       dates and both members:  vor 3.7e-12,  t 3.4e-12,  tr 4.2e-12,  ps 8.9e-14.
     whole field  32 nu_f <= 1e-10 for the five prognostics and the 17 surface and flux fields.  Observed worst 1.75e-11 (ssrd,
       1 July; tsr 1.5e-11, evap 8.3e-12, hfluxn 7.3e-12); the prognostics <= 1.7e-12 (div).  The flat 1e-11 of the older
       whole-field tests would not be safe for the radiative fluxes on a developed state.
   div is NOT admissible per band: its 32 nu is 7.2e-12 ... 1.01e-11 for the fixture state and 1.02e-11 ... 1.39e-11 for the
   perturbed member with these 4 draws, over the cap on 1 October (with 8 draws on the fixture state: up to 1.05e-11; 6.3e-12
   already after one step).  The worst bands are l = 30 of levels 1-2, where the band is tiny next to its rounding noise;
   restricted to l <= 28 it is still 5.4e-12 ... 8.8e-12, too close to the cap to rely on.  So div is held by whole field here
   as in tests/test_model_vs_oracle_gpu.py, and the divergent wind in motion stays with tests/test_step_bands_gpu.py."""
import os

import numpy as np
import pytest

import band_norms as bn
import season_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = list(sc.DATES)
BAND_NAMES = ("vor", "t", "tr", "ps")


@pytest.fixture(scope="module")
def bc():
    return np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return {tag: sc.load(golden_dir, tag) for tag in TAGS}


def test_layout_and_size_of_the_fixture_files(golden_dir, fixtures):
    for tag in TAGS:
        fix = fixtures[tag]
        assert tuple(fix["date"]) == sc.DATES[tag][0]
        assert {k for k in fix if k.startswith("restart_")} == {"restart_" + n for n in sc.RESTART} and len(sc.RESTART) == 19
        for group in ("ref12", "ref36"):
            stored = {k[len(group) + 1:] for k in fix if k.startswith(group + "_")}
            assert stored == set(sc.FIELDS + sc.ZONAL + ("cal_ymdhm", "cal_month_idx")), (tag, group)
        for n in sc.SPEC:
            assert fix["ref12_" + n].shape == ((31, 32, 2) if n == "ps" else (31, 32, 8, 2)), n  # both time levels
        for group in sc.GROUPS:
            for part in ("spec", "surf"):
                assert os.path.getsize(sc.path(golden_dir, tag, group, part)) < sc.MAX_FILE_BYTES


@pytest.mark.parametrize("tag", TAGS)
def test_restarted_oracle_equals_the_reference_bitwise(oracle, bc, fixtures, tag):
    fix = fixtures[tag]
    m = sc.oracle_model(oracle, bc, fix)
    assert m.get("current_step") == 0
    done = 0
    for steps in (12, 36):
        while done < steps:
            assert m.step() == 0
            done += 1
        got = sc.snapshot(m)
        different = []
        for name in sc.FIELDS + sc.ZONAL:
            ref = fix["ref%d_%s" % (steps, name)]
            assert got[name].shape == ref.shape, (name, got[name].shape, ref.shape)
            if not np.array_equal(got[name], ref):
                different.append("%s %.3e" % (name, bn.whole_field(got[name], ref)))
        assert not different, "%s after %d steps: differs from the reference (scaled max error): %s" % (tag, steps, ", ".join(different))
        assert list(got["cal_ymdhm"]) == list(fix["ref%d_cal_ymdhm" % steps])
        assert int(got["cal_month_idx"]) == int(fix["ref%d_cal_month_idx" % steps])
    y, mo, d = sc.DATES[tag][0]
    assert list(got["cal_ymdhm"]) == [y, mo, d + 1, 0, 0]


NORTH = slice(24, 48)  # latitude index, south to north


@pytest.mark.parametrize("tag", TAGS)
def test_the_fixture_is_a_developed_state(oracle, bc, fixtures, tag):
    """Parity on these states means something only if they are what the module docstring says.  Observed figures in the order
    1 April, 1 July, 1 October."""
    fix = fixtures[tag]
    rest = np.load(os.path.join(ROOT, "tests", "golden", "run.npz"))
    # in motion: the vorticity of the developed jets against the start-up transient one day after rest (run.npz: 8.9e-7 1/s)
    vor = np.abs(fix["restart_vor"]).max()
    assert np.abs(rest["d1_vor"]).max() < 1e-6 and vor > 5e-6, vor                     # 7.37e-6, 9.16e-6, 8.02e-6
    assert np.abs(fix["restart_div"]).max() > 5e-7                                    # 7.3e-7, 8.5e-7, 7.2e-7
    # convection is active
    assert (fix["ref12_precnv"] > 0).sum() > 100                                       # 175, 185, 186 columns
    assert (fix["ref12_precls"] > 0).sum() > 100                                       # 2148, 2175, 2268
    # snow and ice are present ...
    snow, ice = fix["ref12_snowc"] > 0, fix["ref12_sice_am"] > 0
    assert snow.sum() > 1000 and ice.sum() > 900, (snow.sum(), ice.sum())              # snow 1401, 1277, 1376; ice 1092, 1117, 1067
    assert ice[:, NORTH].sum() > 300 and ice[:, :24].sum() > 150                       # N 688, 602, 561; S 404, 515, 506
    # ... and the slab memory matters: the land model is away from the climatology it relaxes to
    m = sc.oracle_model(oracle, bc, fix)
    assert np.abs(m.get("stl_lm") - m.get("stlcl_obs")).max() > 1.0                    # 3.05, 3.29, 2.75 K
    assert np.abs(m.get("sst_om") - m.get("sstcl_ob")).max() > 0.5                     # 0.77, 0.75, 1.58 K
    # both sea-ice branches of the coupler's climatology step are populated (orc_model.c: sstcl_ob above / at the freezing point)
    sstfr = float(np.float32(273.2) - np.float32(1.8))
    sea = m.get("fmask_sea") > 0
    sst, sice = m.get("sstcl_ob"), m.get("sicecl_ob")
    above = sea & (sst > sstfr) & (sice > 0) & (sice <= 0.5)
    frozen = sea & (sst == sstfr) & (sice >= 0.5)
    assert above.sum() > 100 and frozen.sum() > 100, (above.sum(), frozen.sum())       # above 366, 809, 378; frozen 726, 308, 689


def test_the_three_states_differ_by_season(fixtures):
    snow = {tag: fixtures[tag]["ref12_snowc"] > 0 for tag in TAGS}
    ice = {tag: fixtures[tag]["ref12_sice_am"] for tag in TAGS}
    assert snow["0701"][:, NORTH].sum() < snow["1001"][:, NORTH].sum() < snow["0401"][:, NORTH].sum()   # 688 < 810 < 846 points
    # sea-ice fraction summed over the hemisphere: summer melt in the north, winter growth in the south
    assert max(ice["0701"][:, NORTH].sum(), ice["1001"][:, NORTH].sum()) < 0.7 * ice["0401"][:, NORTH].sum()  # 223, 310 < 494
    assert ice["0401"][:, :24].sum() < 0.5 * ice["0701"][:, :24].sum() < 0.5 * ice["1001"][:, :24].sum()    # 113, 235, 266
    solar = {tag: fixtures[tag]["ref12_flux_solar_in"] for tag in TAGS}
    assert solar["0701"][-1] > 400 and solar["0701"][0] == 0 and solar["1001"][0] > 0                   # polar day / night: 519, 0, 72.8 W/m2


@pytest.mark.parametrize("member", (0, 1))
@pytest.mark.parametrize("tag", TAGS)
def test_admissibility_of_the_bounds_by_the_oracle_alone(oracle, bc, fixtures, tag, member):
    """Both conditions of the module docstring, for the fixture state and the perturbed member of the GPU tier."""
    fix = fixtures[tag]
    c = sc.case(oracle, bc, fix, tag, member)
    if member:
        t0 = fix["restart_t"]
        moved = np.abs(c["t_start"] - t0)[~sc.BEYOND].max() / np.abs(t0).max()
        assert moved > 0 and np.array_equal(c["t_start"][sc.BEYOND], t0[sc.BEYOND]) and np.all(c["t_start"][0].imag == 0)
        assert np.abs(c["ref"]["t"] - fix["ref12_t"]).max() > 1e-9 * np.abs(fix["ref12_t"]).max()  # a different state
    else:  # the case's reference IS the reference
        assert all(np.array_equal(c["ref"][n], fix["ref12_" + n]) for n in sc.FIELDS)
    # band 31 of t: written by no step, bit for bit
    assert np.array_equal(c["ref"]["t"][sc.BEYOND], c["t_start"][sc.BEYOND]) and np.abs(c["t_start"][sc.BEYOND]).max() > 1e-5
    lines = []
    for name in BAND_NAMES:
        excess = bn.cap_excess(c["nu"][name])
        lines.append("%s member %d: 32 nu of %s per band %.2e" % (tag, member, name, excess))
        assert excess <= bn.CAP, lines[-1]
    lines.append("%s member %d: 32 nu of div per band %.2e (not asserted: module docstring)" % (tag, member, bn.cap_excess(c["nu"]["div"])))
    for name in sc.FIELDS:
        nu_f = bn.MARGIN * c["nu_f"][name]
        lines.append("%s member %d: 32 nu_f of %s %.2e" % (tag, member, name, nu_f))
        assert nu_f <= sc.FIELD_CAP, lines[-1]
    print("\n".join(lines))
