"""Helper of the season tests (not a test): the reference's own developed state on 1 April, 1 July and 1 October 1982
(tests/golden/season_<mmdd>_*.npz, oracle/gen_golden_seasons.py), the recipe that restarts a model from it, the perturbed second
member and the oracle's rounding sensitivity on these states.  Shared by oracle/gen_golden_seasons.py (the reference),
tests/test_seasons_oracle.py (the oracle) and tests/test_seasons_gpu.py (the device).

The fixture of one date is a dict with three groups of keys:

  restart_<name>   the 19 arrays of RESTART: what carries the model's memory across a step boundary at midnight
  ref12_<name>, ref36_<name>   the reference 12 and 36 steps later: the prognostics (both time levels), the fields of SURFACE,
                   the five zonal forcing profiles of ZONAL as one meridian [48], `cal_ymdhm` [5] and `cal_month_idx`
  date             (year, month, day)

No committed file may exceed 1 MiB, so each group is stored as two files, `_spec` (the five prognostics) and `_surf` (the rest):
six files per date, read back into one dict by `load`.

The restart recipe, the same for the reference, the oracle and the device: a fresh model, the boundary fields, `init` at the
fixture's date at 00:00, the RESTART arrays through the ordinary `set`, then steps.  `init` leaves current_step = 0, which has
the phase of the uninterrupted run's step count for the shortwave cycle (mod 3) and the daily forcing (mod 36); the month index
restarts at 1, so the calendar stored with ref12 / ref36 is that of the RESTARTED reference (its date is asserted equal to the
uninterrupted run's by the generator)."""
import os

import numpy as np

import band_norms as bn

SPEC = ("vor", "div", "t", "tr", "ps")
RESTART = SPEC + ("stl_lm", "sst_om", "tice_om", "sice_om", "land_temp", "sst_am", "tice_am", "sice_am", "snow_depth",
                  "soil_avail_water", "hfluxn", "ssrd", "shf", "evap")
SURFACE = ("land_temp", "sst_am", "tice_am", "sice_am", "stl_lm", "sst_om", "tice_om", "snowc", "alb_surface", "olr", "precnv",
           "precls", "tsr", "ssrd", "hfluxn", "shf", "evap")
ZONAL = ("flux_solar_in", "flux_ozone_lower", "flux_ozone_upper", "zenit_correction", "stratospheric_correction")
FIELDS = SPEC + SURFACE  # compared by whole field

# tag -> (date, days since 1982-01-01 in the model's 365-day year)
DATES = {"0401": ((1982, 4, 1), 90), "0701": ((1982, 7, 1), 181), "1001": ((1982, 10, 1), 273)}
GROUPS = ("restart", "ref12", "ref36")
MAX_FILE_BYTES = 1 << 20

NOISE_DRAWS = 4
FIELD_CAP = 1e-10     # on 32 nu_f: the whole-field figure tests/test_calendar_gpu.py accepts for runs of up to 180 steps
FIELD_FLOOR = 1e-12   # whole-field bound = max(32 nu_f, FIELD_FLOOR)
PERTURBATION = 1e-6   # relative amplitude of member 1's temperature perturbation
BEYOND = np.add.outer(np.arange(31), np.arange(32)) >= 31  # band 31 and what lies beyond it


def part_of(key):
    """'spec' or 'surf': the file of its group that holds `key` ('<group>_<name>')."""
    return "spec" if key.split("_", 1)[1] in SPEC else "surf"


def path(gold_dir, tag, group, part):
    return os.path.join(gold_dir, "season_%s_%s_%s.npz" % (tag, group, part))


def load(gold_dir, tag):
    out = {}
    for group in GROUPS:
        for part in ("spec", "surf"):
            with np.load(path(gold_dir, tag, group, part)) as f:
                out.update({k: f[k] for k in f.files})
    return out


def restart(model, fix, member=None):
    """Step 3 of the recipe on anything with the registry's `set`: an oracle.Model or RefModel (member None), or one member of
    an EnsembleModel."""
    for name in RESTART:
        if member is None:
            model.set(name, fix["restart_" + name])
        else:
            model.set(name, fix["restart_" + name], member)


def oracle_model(oracle, bc, fix, state=None):
    """An oracle.Model restarted by the recipe; `state`: prognostic arrays that replace the fixture's afterwards."""
    m = oracle.Model()
    m.set_bc(bc)
    assert m.init(*[int(v) for v in fix["date"]]) == 0
    restart(m, fix)
    for name, value in (state or {}).items():
        m.set(name, value)
    return m


def member_state(fix, member):
    """The prognostics of member 0 (the fixture's) or member 1: t times 1 + PERTURBATION N(0, 1) from default_rng(1), both time
    levels independently; the zonal-mean coefficients keep a zero imaginary part.  Band 31 of t keeps the fixture's value: its
    two time levels are equal, which is why the steps leave it alone (tests/test_model_vs_oracle_gpu.py), and the tests assert
    that they do."""
    state = {n: fix["restart_" + n].copy() for n in SPEC}
    if member:
        f = 1.0 + PERTURBATION * np.random.default_rng(member).standard_normal(state["t"].shape)
        f[BEYOND] = 1.0
        state["t"] = state["t"] * f
        state["t"][0] = state["t"][0].real
    return state


def moved_state(state, draw):
    """Every element of the five prognostics multiplied by bn.ulp_factors from default_rng(draw), in the order of SPEC."""
    rng = np.random.default_rng(draw)
    return {n: state[n] * bn.ulp_factors(rng, state[n].shape) for n in SPEC}


def without_band31(name, a):
    if name != "t":
        return a
    a = a.copy()
    a[BEYOND] = 0.0
    return a


def zonal_column(model, name):
    field = model.get(name)
    assert np.all(field == field[:1, :]), name
    return field[0].copy()


def snapshot(model):
    """FIELDS, ZONAL (one meridian) and the calendar of an oracle.Model as a dict."""
    out = {n: model.get(n) for n in FIELDS}
    out.update({n: zonal_column(model, n) for n in ZONAL})
    ymdhm, month_idx = model.calendar()[:2]
    out["cal_ymdhm"], out["cal_month_idx"] = np.array(ymdhm, dtype=np.int32), np.int32(month_idx)
    return out


_cases = {}


def case(oracle, bc, fix, tag, member, steps=12):
    """The oracle on member `member` of date `tag`, computed once per session and shared (read-only):
      ref     snapshot after `steps` steps
      nu      name -> per level, time level and band, the largest bn.band_errors between ref and NOISE_DRAWS runs from
              moved_state (band 31 of t left out), for the five prognostics
      nu_f    name -> the largest max|moved - ref| / max|ref| over the same runs, for every name of FIELDS
      t_start the temperature before the first step"""
    key = (tag, member, steps)
    if key in _cases:
        return _cases[key]
    state = member_state(fix, member)
    runs = [oracle_model(oracle, bc, fix, state)] + [oracle_model(oracle, bc, fix, moved_state(state, d)) for d in range(NOISE_DRAWS)]
    for m in runs:
        for _ in range(steps):
            assert m.step() == 0
    ref = snapshot(runs[0])
    nu = {n: np.zeros(ref[n].shape[2:] + (32,)) for n in SPEC}
    nu_f = {n: 0.0 for n in FIELDS}
    for m in runs[1:]:
        for n in FIELDS:
            moved = m.get(n)
            nu_f[n] = max(nu_f[n], float(bn.whole_field(moved, ref[n])))
            if n in SPEC:
                nu[n] = np.maximum(nu[n], bn.band_errors(without_band31(n, moved), without_band31(n, ref[n])))
    _cases[key] = {"ref": ref, "nu": nu, "nu_f": nu_f, "t_start": state["t"]}
    return _cases[key]


def field_bound(nu_f):
    return max(bn.MARGIN * nu_f, FIELD_FLOOR)
