"""The arbiter of the derived-field tests: a plain numpy fp64 restatement of the definitions in their stated
order, independent of the kernel.  Inputs in export units: u, v, t, q, vor, div as [..., 8, lat, lon] (level 0 the top), ps
[..., lat, lon] in Pa, px and py (the components of grad ln ps) [..., lat, lon], levels in Pa.  Every sum over the levels is
sequential from k = 0 and its first term starts it."""
import math
import os

import numpy as np

# the reference's own vertical tables (geometry.f90, evaluated in fp32): its table file, not the library's constants
_T = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tables.npz"))
FSG, DHS = _T["fsg"].astype(np.float64), _T["dhs"].astype(np.float64)
SIGL = np.log(FSG)
GRAV = float(np.float32(9.81))
P0 = float(np.float32(1.0e5))
AKAP = float(np.float32(2.0) / np.float32(7.0))  # physical_constants.f90: evaluated in fp32

GRID8 = ("vor_grid", "div_grid", "omega_grid", "rh_grid", "theta_grid")
COLUMN = ("tcwv", "ivt_u", "ivt_v", "ke_col")
PLEV = ("omega_plev", "vor_plev", "div_plev", "rh_plev", "theta_plev")
NAMES = GRID8 + COLUMN + PLEV


def _lev(x, k):
    return np.take(x, k, axis=-3)


def _column_sum(term):
    """term(k) -> the sum over k = 0 ... 7, sequential, the first term starting it"""
    s = term(0)
    for k in range(1, 8):
        s = s + term(k)
    return s


def _exp(x):
    """the C library's exp, element by element (numpy's own exp is another implementation: up to 1 ulp away)"""
    return np.frompyfunc(math.exp, 1, 1)(x).astype(np.float64)


def qsat(t, p):
    """humidity.f90:44-76 (fp32 literals widened): t in K, p = sigma ps in units of p0 -> g/kg"""
    f = lambda x: float(np.float32(x))
    e0, c1, c2, t0, t1, t2 = 6.108e-3, f(17.269), f(21.875), f(273.16), f(35.86), f(7.66)
    t = np.asarray(t, dtype=np.float64)
    warm = t >= t0
    e = np.where(warm, e0 * _exp(c1 * (t - t0) / (t - t1)), e0 * _exp(c2 * (t - t0) / (t - t2)))
    return f(622.0) * e / (p - f(0.378) * e)


def omega(u, v, div, ps, px, py):
    ubar = _column_sum(lambda k: _lev(u, k) * DHS[k])
    vbar = _column_sum(lambda k: _lev(v, k) * DHS[k])
    dbar = _column_sum(lambda k: _lev(div, k) * DHS[k])
    dlnps = -ubar * px - vbar * py - dbar
    sd = np.zeros_like(ps)
    planes = []
    for k in range(8):
        puv = (_lev(u, k) - ubar) * px + (_lev(v, k) - vbar) * py
        sd_next = sd - DHS[k] * (puv + _lev(div, k) - dbar)
        planes.append(ps * (FSG[k] * (dlnps + _lev(u, k) * px + _lev(v, k) * py) + 0.5 * (sd + sd_next)))
        sd = sd_next
    return np.stack(planes, axis=-3)


def omega_scale(u, v, div, ps, px, py):
    """the size of the terms that cancel in omega: ps sum_k dhs[k] (|u px| + |v py| + |D|), per column"""
    return ps * _column_sum(lambda k: DHS[k] * (np.abs(_lev(u, k) * px) + np.abs(_lev(v, k) * py) + np.abs(_lev(div, k))))


def to_levels(x, ps, levels_pa):
    """the sigma-level field at the target pressures: linear in ln p inside the full levels, level 0 above, level 7 below"""
    planes = []
    for p in levels_pa:
        s = np.log(p / ps)
        k = np.clip(np.searchsorted(SIGL, s, side="right") - 1, 0, 6)
        w = (s - SIGL[k]) / (SIGL[k + 1] - SIGL[k])
        pick = lambda kk: np.take_along_axis(x, np.expand_dims(kk, -3), axis=-3).squeeze(-3)
        inside = pick(k) + w * (pick(k + 1) - pick(k))
        planes.append(np.where(s < SIGL[0], _lev(x, 0), np.where(s > SIGL[7], _lev(x, 7), inside)))
    return np.stack(planes, axis=-3)


def derive_reference(fields, ps, px, py, levels_pa=()):
    u, v, t, q, vor, div = (fields[n] for n in ("u", "v", "t", "q", "vor", "div"))
    sig = FSG.reshape((8, 1, 1))
    psk = np.expand_dims(ps, -3)
    out = {"vor_grid": vor, "div_grid": div, "omega_grid": omega(u, v, div, ps, px, py)}
    out["rh_grid"] = (q * 1000.0) / qsat(t, sig * (psk / P0))
    out["theta_grid"] = t * (P0 / (sig * psk)) ** AKAP
    psg = ps / GRAV
    out["tcwv"] = psg * _column_sum(lambda k: _lev(q, k) * DHS[k])
    out["ivt_u"] = psg * _column_sum(lambda k: _lev(q, k) * _lev(u, k) * DHS[k])
    out["ivt_v"] = psg * _column_sum(lambda k: _lev(q, k) * _lev(v, k) * DHS[k])
    out["ke_col"] = psg * _column_sum(lambda k: 0.5 * (_lev(u, k) * _lev(u, k) + _lev(v, k) * _lev(v, k)) * DHS[k])
    if len(levels_pa):
        for name in PLEV:
            out[name] = to_levels(out[name.replace("_plev", "_grid")], ps, levels_pa)
    return out
