"""The arbiter of the spectra tests: numpy fp64, written from the definition, sharing nothing with csrc/.

Fields come in the reference's shape, complex (31 m, 32 n[, 8 levels]) of ONE time level; elm2 is the (31, 32) table a^2 / (l (l + 1))
of the golden tables or of the oracle.  The total wavenumber of element (m, n) is l = m + n; a bin sums w_m |f|^2 over m ascending
(w_0 = 1, w_m = 2 otherwise); elements with m + n > 31 take no part."""
import numpy as np

NAMES = ("ke_rot_spectrum", "ke_div_spectrum", "t_spectrum", "q_spectrum", "lnps_spectrum", "t_mean", "q_mean", "lnps_mean")
ROOT_HALF = 0.70710678118654752440


def bin_sums(f):
    """S_l = sum_m w_m |f_l^m|^2 for l = 0 ... 31 -> [32] (or [8][32] for a field with levels)."""
    f = np.asarray(f, dtype=np.complex128)
    out = np.zeros((32,) + f.shape[2:])
    for l in range(32):
        s = np.zeros(f.shape[2:])
        for m in range(0, min(l, 30) + 1):
            c = f[m, l - m]
            p = c.real * c.real + c.imag * c.imag
            s = s + (p if m == 0 else 2.0 * p)
        out[l] = s
    return np.moveaxis(out, 0, -1)


def elm2_of_l(elm2):
    return np.array([np.asarray(elm2)[0, l] for l in range(32)])


def spectra(vor, div, t, tr, ps, elm2):
    """dict name -> fp64 array ([8][32], [32], [8] or [1]) of one member's state at one time level."""
    e = elm2_of_l(elm2)
    return {
        "ke_rot_spectrum": 0.25 * (e * bin_sums(vor)),
        "ke_div_spectrum": 0.25 * (e * bin_sums(div)),
        "t_spectrum": 0.5 * bin_sums(t),
        "q_spectrum": 0.5 * bin_sums(tr),
        "lnps_spectrum": 0.5 * bin_sums(ps),
        "t_mean": np.asarray(t)[0, 0].real * ROOT_HALF,
        "q_mean": np.asarray(tr)[0, 0].real * ROOT_HALF,
        "lnps_mean": np.array([np.asarray(ps)[0, 0].real * ROOT_HALF]),
    }


def area_mean(grid, wt):
    """Gaussian-weighted global mean of a (96, 48) grid field: wt holds the 24 weights of one hemisphere (they sum to 1), the same
    for both."""
    zonal = np.asarray(grid).mean(axis=0)
    w = np.asarray(wt)
    assert zonal.shape == (48,) and w.shape == (24,)
    return float(0.5 * ((zonal[:24] * w).sum() + (zonal[:23:-1] * w).sum()))
