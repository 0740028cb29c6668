"""The arbiter of the pressure-level tests: a plain numpy fp64 restatement of the definition, independent of
the kernel.  Inputs in export units: u, v, t, q, z as [..., 8, lat, lon] (level 0 the top), ps [..., lat, lon] in Pa, phis0
[..., lat, lon] in m^2/s^2, levels in Pa.  Returns u_plev ... z_plev as [..., n, lat, lon] and mslp [..., lat, lon]."""
import os

import numpy as np

# the reference's own full-level sigmas (geometry.f90, evaluated in fp32): its table file, not the library's constants
FSG = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tables.npz"))["fsg"].astype(np.float64)
SIGL = np.log(FSG)
RGAS = float(np.float32(2.0) / np.float32(7.0)) * 1004.0   # physical_constants.f90: akap * cp, fp32 literals widened
GRAV = float(np.float32(9.81))
GAMMA = 6.0 / 1000.0                                        # K/m
KAPPA = RGAS * GAMMA / GRAV


def plev_reference(fields, ps, phis0, levels_pa):
    lev = lambda x, k: np.take(x, k, axis=-3)
    out = {name + "_plev": [] for name in fields}
    t, z = fields.get("t"), fields.get("z")
    for p in levels_pa:
        s = np.log(p / ps)
        k = np.clip(np.searchsorted(SIGL, s, side="right") - 1, 0, 6)  # sigl[k] <= s < sigl[k+1]; the last layer closed above
        w = (s - SIGL[k]) / (SIGL[k + 1] - SIGL[k])
        top, below = s < SIGL[0], s > SIGL[7]
        pick = lambda x, kk: np.take_along_axis(x, np.expand_dims(kk, -3), axis=-3).squeeze(-3)
        for name, x in fields.items():
            inside = pick(x, k) + w * (pick(x, k + 1) - pick(x, k))
            if name == "t":
                low = lev(t, 7) * np.exp(KAPPA * (s - SIGL[7]))
                high = lev(t, 0)
            elif name == "z":
                t_low = lev(t, 7) * np.exp(KAPPA * (s - SIGL[7]))
                low = lev(z, 7) - (t_low - lev(t, 7)) / GAMMA
                high = lev(z, 0) + (RGAS / GRAV) * lev(t, 0) * (SIGL[0] - s)
            else:
                low, high = lev(x, 7), lev(x, 0)
            out[name + "_plev"].append(np.where(top, high, np.where(below, low, inside)))
    out = {name: np.stack(planes, axis=-3) for name, planes in out.items()}
    if t is not None and phis0 is not None:
        t_s = lev(t, 7) * np.exp(-KAPPA * SIGL[7])
        out["mslp"] = ps * (1.0 + GAMMA * (phis0 / GRAV) / t_s) ** (GRAV / (RGAS * GAMMA))
    return out
