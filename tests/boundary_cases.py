"""Helper of the boundary-set tests (not a test): three boundary-field sets derived from the example file, physically sane enough
to be STEPPED, and what tests/test_boundary_cases_cpu.py (the oracle alone), tests/test_boundaries_oracle.py (oracle against
reference, goldens of oracle/gen_golden_boundaries.py) and tests/test_boundaries_gpu.py (device against oracle) share.

Everything else that compares a stepping model with the oracle or the reference runs on the example planet: one land-sea mask,
one ice edge, one snow cover, one orography.  The sets of oracle/init_cases.py and the random sets of tests/test_init_gpu.py
exercise `init` and cannot be stepped (`holes` gives NaN in sst_am, tice_am and land_temp within 72 oracle steps).

The example marks missing values with 9.97e36, which fill_missing_values (boundaries.f90:69-113, `value < 0`) does not treat as
missing: they hide behind the mask only while the mask is the example's.  `demiss` replaces every value > 1e30 by -999 in stl
and sst -- the model's own fill_missing_values then fills them, so a stepping model runs on filled points -- and by 0 in snowd,
swl1..3, icec, alb, vegh and vegl.

  mirrored   every 2-D or 3-D array v becomes roll(v[:, ::-1], 37, axis 0), the 3-D ones also rolled by 6 months: the ice cap,
             the high orography and the seasons on the other side, nothing aligned with a longitude block.  No demiss: the
             mirrored mask still hides the marks.
  icy        demiss; sst -= 4 K where valid; icec = clip(1.6 icec + 0.2 [0 < sst < 277], 0, 1) with the shifted sst;
             snowd * 3; alb = min(alb + 0.1, 0.8): both branches of the coupler's sea-ice step well populated.
  patchy     demiss; lsm = clip(0.15 + 0.7 lsm + 0.1 sin(0.9 i) cos(0.7 j), 0, 1): fractional land nearly everywhere; vegh and
             vegl swapped; swl1..3 * 0.5; orog * 1.3.

All sets are fp64 dicts under the example file's keys; the 1-D lon / lat pass through unchanged."""
import os

import numpy as np

import band_norms as bn
from test_model_vs_oracle_gpu import BEYOND, SPEC, SURF, perturbation  # (shared with the six-member test, unchanged there)

SETS = ("mirrored", "icy", "patchy")
# the second date crosses midnight and a month boundary inside 12 steps: one call holds re-used and fresh couplings and a new month_idx
START_DATES = ((1982, 1, 1, 0, 0), (1982, 6, 30, 20, 0))
N_MONTHS = 2  # planes of sst_anom: n_months + 2 (30 June + 12 steps reads July's)
MISSING = 1e30

# compared by whole field on top of SPEC and SURF; every name is held by both registries (oracle/orc_model.c, pyspeedy_amd/registry.py)
MORE = ("sst_om", "tice_om", "ssti_om", "stl_lm", "snow_depth", "soil_avail_water", "sstan_am", "evap")
SURFACE = SURF + MORE
FIELDS = SPEC + SURFACE
EXACT_FORMS = FIELDS + ("rad_tau2", "olr")


def tag(start):
    return "%02d%02d" % (start[1], start[2])


def golden_path(gold_dir, name, start, part):
    """tests/golden/bounds_<set>_<mmdd>_<spec|surf>.npz: the reference after 12 unperturbed steps (oracle/gen_golden_boundaries.py)."""
    return os.path.join(gold_dir, "bounds_%s_%s_%s.npz" % (name, tag(start), part))


def example(bc):
    return {k: np.array(bc[k], dtype=np.float64) for k in bc.files}


def demiss(b):
    for k in ("stl", "sst"):
        b[k][b[k] > MISSING] = -999.0
    for k in ("snowd", "swl1", "swl2", "swl3", "icec", "alb", "vegh", "vegl"):
        b[k][b[k] > MISSING] = 0.0
    return b


def mirrored(bc):
    b = example(bc)
    for k, v in b.items():
        if v.ndim >= 2:
            v = np.roll(v[:, ::-1], 37, axis=0)
            b[k] = np.ascontiguousarray(np.roll(v, 6, axis=2) if v.ndim == 3 else v)
    return b


def icy(bc):
    b = demiss(example(bc))
    sst = b["sst"]
    sst[sst > 0] -= 4.0
    b["icec"] = np.clip(1.6 * b["icec"] + 0.2 * ((sst < 277) & (sst > 0)), 0, 1)
    b["snowd"] *= 3
    b["alb"] = np.minimum(b["alb"] + 0.1, 0.8)
    return b


def patchy(bc):
    b = demiss(example(bc))
    i, j = np.arange(96)[:, None], np.arange(48)[None, :]
    b["lsm"] = np.clip(0.15 + 0.7 * b["lsm"] + 0.1 * np.sin(0.9 * i) * np.cos(0.7 * j), 0, 1)
    b["vegh"], b["vegl"] = b["vegl"], b["vegh"]
    for k in ("swl1", "swl2", "swl3"):
        b[k] *= 0.5
    b["orog"] *= 1.3
    return b


_BUILDERS = {"example": example, "mirrored": mirrored, "icy": icy, "patchy": patchy}
_sets = {}


def fields(bc, name):
    """The set `name` ("example" or one of SETS), built once per session from the example file `bc`: treat as read-only."""
    if name not in _sets:
        _sets[name] = _BUILDERS[name](bc)
    return _sets[name]


def anomaly():
    """A smooth SST anomaly of up to 1.5 K on the N_MONTHS + 2 planes, for the cases that switch the anomaly on."""
    i, j, k = np.arange(96)[:, None, None], np.arange(48)[None, :, None], np.arange(N_MONTHS + 2)[None, None, :]
    return 1.5 * np.sin(2 * np.pi * i / 96 + 0.7 * k) * np.cos(np.pi * (j - 23.5) / 48) - 0.3


def oracle_model(oracle, b, start, sst_anom=None):
    """An oracle.Model on the set `b`, initialised at `start`."""
    m = oracle.Model(n_months=N_MONTHS)
    m.set_bc(b, sst_anom)
    assert m.init(*start) == 0
    return m


def set_member(ens, b, member):
    """The boundary fields of the set `b` into one member (-1: every member) of an EnsembleModel; `init` is the caller's."""
    from pyspeedy_amd.model import BC_MAP
    for state_name, key in BC_MAP:
        ens.set(state_name, b[key], member)


def get(model, name, member=None):
    """`name` of an oracle.Model (member None) or of one member of an EnsembleModel; hfluxn on the planes the reference writes."""
    a = model.get(name) if member is None else model.get(name, member)
    return a[:, :, :2] if name == "hfluxn" else a


def noisy_runs(oracle, b, start, t, draws=bn.NOISE_DRAWS):
    """`draws` oracle models of the same case whose temperature `t` is moved by one-ulp factors after `init`: the oracle's own
    rounding sensitivity, as tests/test_model_vs_oracle_gpu.py measures it."""
    runs = []
    for draw in range(draws):
        m = oracle_model(oracle, b, start)
        m.set("t", t * bn.ulp_factors(np.random.default_rng(draw), (31, 32, 8, 2)))
        runs.append(m)
    return runs


class Held:
    """Arrays by name behind the `get` of a model (a copy each time), so that stored results can stand where
    tests/test_model_vs_oracle_gpu.check_bands expects a live oracle.Model."""

    def __init__(self, arrays):
        self.arrays = arrays

    def get(self, name):
        return self.arrays[name].copy()


MEMBER = {"example": 0, "mirrored": 1, "icy": 2, "patchy": 3}  # the member a set is in the four-planet model; its perturbation's seed
BAND_NAMES = ("t", "tr", "ps")
_cases = {}


def case(oracle, bc, name, start, steps=12):
    """The oracle on the set `name` from `start`, computed once per session and shared (read-only).  The temperature after `init` is
    multiplied by perturbation(MEMBER[name]) (the example, member 0, stays unperturbed), as tests/test_boundaries_gpu.py does.
      stl12, sst12  the filled climatologies after `init`
      t_start       the temperature before the first step
      ref           FIELDS after 12 steps, `noisy`: the same of bn.NOISE_DRAWS runs whose t is moved by one-ulp factors (BAND_NAMES
                    and, as `nu_f`, the largest whole-field move of every name of FIELDS)
      calendar      (ymdhm, month_idx) after the 12 steps
      last          with steps > 12: FIELDS after `steps` steps; `codes` the return codes of all steps"""
    key = (name, tuple(start), steps)
    if key in _cases:
        return _cases[key]
    b = fields(bc, name)
    m = oracle_model(oracle, b, start)
    out = {"stl12": m.get("stl12"), "sst12": m.get("sst12")}
    if MEMBER[name]:
        m.set("t", m.get("t") * perturbation(MEMBER[name]))
    out["t_start"] = m.get("t")
    runs = noisy_runs(oracle, b, start, out["t_start"])
    codes = [m.step() for _ in range(12)]
    for other in runs:
        codes += [other.step() for _ in range(12)]
    out["ref"] = {n: get(m, n) for n in FIELDS}
    out["noisy"] = [Held({n: other.get(n) for n in BAND_NAMES}) for other in runs]
    out["nu_f"] = {n: max(float(bn.whole_field(get(other, n), out["ref"][n])) for other in runs) for n in FIELDS}
    out["calendar"] = tuple(m.calendar()[:2])
    codes += [m.step() for _ in range(steps - 12)]
    out["last"] = {n: get(m, n) for n in FIELDS + ("fmask_land",)}
    out["codes"] = codes
    _cases[key] = out
    return out


def band_nu(c, name):
    """Per level, time level and band the largest move of `name` among the noisy runs of case `c` (band 31 of t left out, as
    check_bands leaves it out)."""
    def cut(a):
        if name == "t":
            a = a.copy()
            a[BEYOND] = 0.0
        return a
    ref = cut(c["ref"][name])
    nu = np.zeros(ref.shape[2:] + (32,))
    for other in c["noisy"]:
        nu = np.maximum(nu, bn.band_errors(cut(other.get(name)), ref))
    return nu
