"""The arbiter of the breeding tests: numpy fp64 and math.fsum, written from the definition, sharing nothing
with csrc/.

A state is a dict name -> complex (31 m, 32 n[, 8 levels], 2 time levels) over vor, div, t, tr, ps, as EnsembleModel.get returns
a member; index 0 of the last axis is time level 1, the level the amplitude reads.  elm2 is the (31, 32) table a^2 / (l (l + 1)) of
the golden tables or of the oracle; weights is a dict name -> (8,) (ps reads entry 0; a name left out weighs nothing).

For D = X_p - X_c on time level 1, w_m = 1 for m = 0 and 2 otherwise, over the coefficients with m + n <= 31:
    E(vor | div, k) = 1/4 sum elm2(m + n) w_m |D|^2      E(t | tr | ps, k) = 1/2 sum w_m |D|^2
    A = sqrt(sum weights[name][k] E(name, k)),  s = target / A,  X_p' = X_c + s (X_p - X_c) on both time levels for m + n <= 31."""
import math

import numpy as np

NAMES = ("vor", "div", "t", "tr", "ps")
L = np.add.outer(np.arange(31), np.arange(32))  # total wavenumber of the coefficient (m, n)
INSIDE = L <= 31
W_M = np.where(np.arange(31) == 0, 1.0, 2.0)[:, None]


def plane_terms(name, d, elm2):
    """The non-negative terms of E(name, k) for one plane's difference field d (31, 32): 2 x 527 of them, real parts then
    imaginary parts, with the factors 1/4 elm2 w_m or 1/2 w_m applied."""
    factor = 0.25 * np.asarray(elm2) * W_M if name in ("vor", "div") else 0.5 * W_M * np.ones((31, 32))
    re, im = d.real[INSIDE], d.imag[INSIDE]
    f = factor[INSIDE]
    return np.concatenate([f * (re * re), f * (im * im)])


def energies(xp, xc, elm2):
    """dict name -> [levels] of E(name, k) (math.fsum of the plane's terms)"""
    out = {}
    for n in NAMES:
        d = np.asarray(xp[n])[..., 0] - np.asarray(xc[n])[..., 0]
        planes = [d] if d.ndim == 2 else [d[:, :, k] for k in range(8)]
        out[n] = np.array([math.fsum(plane_terms(n, p, elm2)) for p in planes])
    return out


def weighted_terms(xp, xc, weights, elm2):
    """All terms of A^2: 33 planes x 527 coefficients x 2 parts = 34 782, each with its plane's weight applied"""
    out = []
    for n in NAMES:
        d = np.asarray(xp[n])[..., 0] - np.asarray(xc[n])[..., 0]
        planes = [d] if d.ndim == 2 else [d[:, :, k] for k in range(8)]
        w = np.atleast_1d(np.asarray(weights.get(n, np.zeros(8)), dtype=np.float64))
        for k, p in enumerate(planes):
            out.append(float(w[k]) * plane_terms(n, p, elm2))
    terms = np.concatenate(out)
    assert terms.shape == (33 * 527 * 2,) and (terms >= 0).all()
    return terms


def amplitude(xp, xc, weights, elm2):
    return math.sqrt(math.fsum(weighted_terms(xp, xc, weights, elm2)))


def rescale_variable(xp, xc, s):
    """One variable of a bred member, both time levels: the numpy line on real and imaginary parts for m + n <= 31; every operation
    is rounded on its own.  s must be a numpy float64 (or a Python float)."""
    xp, xc = np.asarray(xp), np.asarray(xc)
    new = np.empty_like(xp)
    new.real = xc.real + s * (xp.real - xc.real)
    new.imag = xc.imag + s * (xp.imag - xc.imag)
    out = xp.copy()
    out[INSIDE] = new[INSIDE]
    return out


def rescale(xp, xc, s):
    """dict name -> the rescaled variable of the bred member"""
    return {n: rescale_variable(xp[n], xc[n], s) for n in NAMES}
