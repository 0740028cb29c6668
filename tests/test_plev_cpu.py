"""CPU tier of the pressure-level fields: pins the numpy restatement of the definition (tests/plev_reference.py, the arbiter of
tests/test_plev_gpu.py) on analytic columns and on the reference's own one-day state, and checks that the four new procedures
are declared and exported.  No compute entry point is called here (no GPU in this tier)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from plev_reference import FSG, GAMMA, GRAV, KAPPA, RGAS, SIGL, plev_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPA = 100.0
LEVELS = [925.0, 850.0, 700.0, 500.0, 300.0, 200.0, 100.0, 30.0, 10.0]  # hPa


def turned(x):  # (lon, lat[, lev]) -> ([lev,] lat, lon)
    return np.ascontiguousarray(x.transpose(*range(x.ndim - 1, -1, -1)))


@pytest.fixture(scope="module")
def day1(golden_dir):
    e, r = np.load(golden_dir + "/export.npz"), np.load(golden_dir + "/run.npz")
    fields = {n: turned(e["d1_%s_grid" % g]) for n, g in (("u", "u"), ("v", "v"), ("t", "t"), ("q", "q"), ("z", "phi"))}
    return fields, turned(e["d1_ps_grid"]), turned(r["d1_phis0"])


def test_full_levels_return_themselves(day1):
    """At p = fsg[k] ps the restatement returns T[k] (to 1 ulp) and Z[k] (to 1e-11 m), for every k."""
    fields, ps, phis0 = day1
    for k in range(8):
        out = plev_reference(fields, ps, phis0, [FSG[k] * ps])
        dt = np.abs(out["t_plev"][0] - fields["t"][k])
        dz = np.abs(out["z_plev"][0] - fields["z"][k]).max()
        print("level %d: max |dT| = %.3g K, max |dZ| = %.3g m" % (k, dt.max(), dz))
        assert (dt <= np.spacing(fields["t"][k])).all()
        assert dz <= 1e-11


def column(values):  # eight level values -> [8, 1, 1]
    return np.asarray(values, dtype=np.float64).reshape(8, 1, 1)


@pytest.mark.parametrize("ps_hpa, zs", [(1013.25, 0.0), (850.0, 1400.0), (600.0, 4200.0)])
def test_isothermal_columns(ps_hpa, zs):
    """Isothermal hydrostatic columns (Z linear in ln p): Z exact to 1e-10 m at every target level that is not below level 7, the
    two above the top full level (30 and 10 hPa) included."""
    t0, ps = 250.0, np.full((1, 1), ps_hpa * HPA)
    z_of = lambda p: zs + (RGAS / GRAV) * t0 * np.log(ps / p)
    fields = {"t": column([t0] * 8), "z": column([z_of(f * ps)[0, 0] for f in FSG])}
    levels = [p * HPA for p in LEVELS if np.log(p * HPA / ps[0, 0]) <= SIGL[7]]
    assert 1000.0 in levels and 3000.0 in levels
    out = plev_reference(fields, ps, np.full((1, 1), zs * GRAV), levels)
    for j, p in enumerate(levels):
        err = abs(out["z_plev"][j, 0, 0] - z_of(p)[0, 0])
        print("ps %.2f hPa, %.0f hPa: |dZ| = %.3g m" % (ps_hpa, p / HPA, err))
        assert err <= 1e-10
        assert out["t_plev"][j, 0, 0] == t0


@pytest.mark.parametrize("ps_hpa, zs", [(1013.25, 0.0), (850.0, 1400.0), (600.0, 4200.0)])
def test_constant_lapse_rate_below_the_lowest_level(ps_hpa, zs):
    """Below level 7 the definition is the constant-lapse-rate profile T = T_s sigma^kappa and its hydrostatic integral: T to 1e-12 K
    and Z to 1e-10 m of the analytic profile at 925, 1000 and 1050 hPa; mslp = ps ((T_s + gamma z_s) / T_s)^(g / R gamma) to 1e-9 Pa,
    and ps bitwise where z_s = 0."""
    t_s, ps = 288.0, np.full((1, 1), ps_hpa * HPA)
    t_of = lambda sigma: t_s * sigma ** KAPPA
    z_of = lambda sigma: zs + (t_s - t_of(sigma)) / GAMMA
    fields = {"t": column([t_of(f) for f in FSG]), "z": column([z_of(f) for f in FSG])}
    levels = [p * HPA for p in (925.0, 1000.0, 1050.0) if np.log(p * HPA / ps[0, 0]) > SIGL[7]]
    assert levels
    out = plev_reference(fields, ps, np.full((1, 1), zs * GRAV), levels)
    for j, p in enumerate(levels):
        sigma = p / ps[0, 0]
        et, ez = abs(out["t_plev"][j, 0, 0] - t_of(sigma)), abs(out["z_plev"][j, 0, 0] - z_of(sigma))
        print("ps %.2f hPa, %.0f hPa: |dT| = %.3g K, |dZ| = %.3g m" % (ps_hpa, p / HPA, et, ez))
        assert et <= 1e-12 and ez <= 1e-10
    # (the surface temperature of the definition is that of the profile only to rounding: T[7] exp(-kappa sigl[7]))
    expect = ps[0, 0] * ((t_s + GAMMA * zs) / t_s) ** (GRAV / (RGAS * GAMMA))
    print("ps %.2f hPa: |d mslp| = %.3g Pa" % (ps_hpa, abs(out["mslp"][0, 0] - expect)))
    assert abs(out["mslp"][0, 0] - expect) <= 1e-9
    if zs == 0.0:
        assert out["mslp"][0, 0] == ps[0, 0]


def test_reference_state_is_plausible(day1):
    """On the reference's one-day state: Z decreases with p at every point; z(sigma = 1) is within 60 m of the ground (the
    reference's geopotential carries its own layer corrections); mslp between 950 and 1050 hPa; Z500 between 5000 and 6000 m."""
    fields, ps, phis0 = day1
    levels = [p * HPA for p in sorted(LEVELS + [1050.0])]
    out = plev_reference(fields, ps, phis0, levels)
    assert (np.diff(out["z_plev"], axis=0) < 0.0).all()
    ground = plev_reference({"t": fields["t"], "z": fields["z"]}, ps, phis0, [ps])["z_plev"][0] - phis0 / GRAV
    print("z(sigma = 1) - z_s: %.1f ... %.1f m, mean %.2f" % (ground.min(), ground.max(), ground.mean()))
    assert np.abs(ground).max() <= 60.0
    print("mslp %.1f ... %.1f hPa" % (out["mslp"].min() / HPA, out["mslp"].max() / HPA))
    assert 950.0 * HPA <= out["mslp"].min() and out["mslp"].max() <= 1050.0 * HPA
    z500 = out["z_plev"][levels.index(500.0 * HPA)]
    print("Z500 %.0f ... %.0f m" % (z500.min(), z500.max()))
    assert 5000.0 <= z500.min() and z500.max() <= 6000.0
    # the order of the caller is kept: the same planes in reverse
    back = plev_reference(fields, ps, phis0, levels[::-1])
    for name in ("u_plev", "v_plev", "t_plev", "q_plev", "z_plev"):
        assert np.array_equal(back[name], out[name][::-1])


NEW_SYMBOLS = ("spd_model_plev_configure", "spd_model_plev_levels", "spd_model_plev_compute", "spd_model_plev_read")


def test_new_symbols_declared_and_exported(hip_lib):
    """The four procedures are declared in include/pyspeedy_amd.h, exported by the built library, bound by ctypes, and have
    Fortran interfaces."""
    import pyspeedy_amd._lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(spd_[a-z0-9_]+)\s*\(", text))
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name + " is not declared in pyspeedy_amd.h"
        assert hasattr(raw, name), "libpyspeedy_amd.so does not export " + name
        assert name in L.EXPORTED_SYMBOLS
        assert 'bind(C, name="%s")' % name in fortran
