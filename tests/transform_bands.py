"""Helper of the transform and operator band tests (not a test): the public spectral path -- spec2grid, grid2spec, the four stage
calls and the spectral operators of ModSpectral -- measured as tests/band_norms.py measures the model step, and the inputs that
tests/test_transform_bands_cpu.py (oracle only), tests/test_transform_bands_gpu.py and tests/test_specops_gpu.py share.

Spectral output: band_norms.band_errors, every total wavenumber l = m + n scaled by its own maximum.  Grid output: one figure
per latitude row, max_i |got - ref| / max_i |ref|.  The bound is band_norms.bound(nu) = clip(32 nu, 1e-13, 1e-11), nu being the
largest change of the ORACLE's result in that band or row over NOISE_DRAWS draws in which every input element moves by at most
one ulp (as band_norms.noise_floor does; MARGIN, FLOOR and CAP are that file's).

Arrays carry the field index first and are in the device's layout: spectra complex [F, 32, 31] (index [n][m]), grids
[F, 48, 96], Fourier planes [F, 48, 62].

Red fields: humidity and temperature of the golden step state, put on the grid by the oracle.  Their spectra fall by four
orders of magnitude from l = 0 to l = 30, which neither white-noise grids nor 1 / (1 + l) spectra do.  Vorticity, divergence
and the temperature's two uppermost levels are left out: 32 nu of grid2spec reaches 5.8e-9 and 1.35e-11 ... 3.3e-11 there, over
the cap (the humidity is zero at those two levels).

Operator inputs: 33 full-rectangle spectra with content in the row n = 31 and in m + n > 31; field b of a batch is
base[b % 33] * 2^((b // 33) % 8 - 4).  The operators are linear and a power of two is exact, so the reference of field b is the
base reference times the same factor, bit for bit, while no two fields of a batch are equal."""
import numpy as np

import band_norms as bn

# (variable, level, time level) of tests/golden/step.npz, 0-based; the list is fixed
RED_FIELDS = tuple(("tr", k, j) for k in range(2, 8) for j in (0, 1)) + tuple(("t", k, 1) for k in range(3, 8))
N_BASE = 33
WHOLE_TOL = 1e-13  # the whole-field rule of tests/test_transforms_gpu.py

_BEYOND = np.add.outer(np.arange(32), np.arange(31)) >= 31  # [n][m]: m + n >= 31


def seeded_spectra(n, seed=1234, triangular=True):
    rng = np.random.default_rng(seed)
    nn, mm = np.meshgrid(np.arange(32), np.arange(31), indexing="ij")
    ll = mm + nn
    s = (rng.standard_normal((n, 32, 31)) + 1j * rng.standard_normal((n, 32, 31))) / (1.0 + ll)
    if triangular:
        s[:, ll > 30] = 0.0
    s[:, :, 0] = s[:, :, 0].real
    return s


# ---- measures ------------------------------------------------------------------------------------------------------------------
def spec_bands(got, ref):
    """[F, 32, 31] -> [F, 32]: band_norms.band_errors of every field (band 31: all of m + n >= 31, by its own maximum)."""
    return bn.band_errors(np.transpose(got, (2, 1, 0)), np.transpose(ref, (2, 1, 0)))


def forward_bands(got, ref):
    """Output of grid2spec / legendre, [F, 32, 31] -> [F, 31]: the bands inside the truncation."""
    return spec_bands(got, ref)[:, :31]


def forward_residue(got, ref):
    """Output of grid2spec / legendre -> [F]: max|got - ref| over m + n >= 31 (quadrature residue, a band like no other: held to
    the whole-field rule) / the field's max|ref|."""
    return np.abs(got - ref)[:, _BEYOND].max(axis=1) / np.abs(ref).max(axis=(1, 2))


def row_errors(got, ref):
    """[F, 48, 96] -> [F, 48]: max_i |got - ref| / max_i |ref| per latitude row (a row of zeros: by the field's maximum)."""
    mag = np.abs(ref).max(axis=2)
    field = mag.max(axis=1, keepdims=True)
    return np.abs(got - ref).max(axis=2) / np.where(mag > 0.0, mag, np.where(field > 0.0, field, 1.0))


def whole_fields(got, ref):
    """[F, ...] -> [F]: the figure of the older tests, per field."""
    axes = tuple(range(1, ref.ndim))
    return np.abs(got - ref).max(axis=axes) / np.maximum(np.abs(ref).max(axis=axes), 1e-300)


def noise_floor(run, inputs, measure):
    """band_norms.noise_floor for a plain function: run(*inputs) -> tuple of arrays.  -> (reference, nu): the result for the inputs
    as they are, and per output the largest measure(moved, reference) over NOISE_DRAWS results, in each of which every element
    of every input is multiplied by band_norms.ulp_factors.  Every field is a case of its own: its factors come from a fresh
    default_rng(draw), drawn in the oracle's Fortran layout of the field, the first input before the second."""
    reference = run(*inputs)
    nu = [np.zeros_like(measure(r, r)) for r in reference]
    for draw in range(bn.NOISE_DRAWS):
        rngs = [np.random.default_rng(draw) for _ in range(inputs[0].shape[0])]
        moved = [x * np.stack([bn.ulp_factors(rng, f.T.shape).T for rng, f in zip(rngs, x)]) for x in inputs]
        for k, out in enumerate(run(*moved)):
            nu[k] = np.maximum(nu[k], measure(out, reference[k]))
    return reference, nu


def report(err, nu, unit="l"):
    """(worst error / bound, text of the ten worst) of err, nu: [F, bands] (unit "l", as band_norms.describe writes them) or
    [F, rows] (unit "row")."""
    rows = bn.worst_bands(err, nu)
    if unit == "l":
        text = bn.describe(rows, ("field",))
    else:
        text = "\n".join("field %d, %s %d: error %.3e, nu %.3e, bound %.3e" % ((r[0], unit) + r[1:]) for r in rows)
    return rows[0][-3] / rows[0][-1], text


# ---- per-field oracle calls in the device's layout -----------------------------------------------------------------------------
def per_field(fn, nout, *arrays):
    """fn on every field (transposed to the oracle's Fortran layout and back) -> tuple of nout stacked arrays."""
    outs = [[] for _ in range(nout)]
    for f in range(arrays[0].shape[0]):
        res = fn(*[a[f].T for a in arrays])
        for k, r in enumerate(res if nout > 1 or isinstance(res, tuple) else (res,)):
            outs[k].append(np.ascontiguousarray(r.T))
    return tuple(np.stack(o) for o in outs)


def oracle_operator(oracle, name):
    """name -> function of stacked device-layout arrays returning a tuple of stacked arrays, by one oracle call per field."""
    table = {
        "vort2vel": lambda a, b: per_field(oracle.vort2vel, 2, a, b),
        "vel2vort": lambda a, b: per_field(oracle.vel2vort, 2, a, b),
        "gradient": lambda a: per_field(oracle.gradient, 2, a),
        "laplacian": lambda a: per_field(oracle.laplacian, 1, a),
        "laplacian_inv": lambda a: per_field(lambda x: oracle.laplacian(x, True), 1, a),
        "truncate": lambda a: per_field(oracle.truncate, 1, a),
    }
    return table[name]


def oracle_stage(oracle, name, x, kcos=1):
    """The stage calls on stacked device-layout arrays, one oracle call per field.  The oracle's Legendre stages see a spectrum
    as the real (62, 32) array (Re, Im interleaved along m) that it is in memory."""
    if name == "legendre_inv":
        return per_field(lambda s: oracle.legendre_inv(np.ascontiguousarray(s.T).view(np.float64).reshape(32, 62).T), 1, x)[0]
    if name == "legendre":
        r = per_field(oracle.legendre, 1, x)[0]  # [F, 32, 62]
        return r[:, :, 0::2] + 1j * r[:, :, 1::2]
    if name == "fourier_inv":
        return per_field(lambda f: oracle.fourier_inv(f, kcos), 1, x)[0]
    if name == "fourier":
        return per_field(oracle.fourier, 1, x)[0]
    raise KeyError(name)


# ---- the cases, computed once per session and shared: treat them as read-only --------------------------------------------------
_cases = {}


def red_spectra(gold):
    return np.stack([np.ascontiguousarray(gold["s0_" + n][:, :, k, j].T) for n, k, j in RED_FIELDS])


def red_name(f):
    return "%s level %d time level %d" % RED_FIELDS[f]


def red_case(oracle, gold):
    """dict: spectra [17, 32, 31]; grids [17, 48, 96] = oracle.spec2grid(spectra, 1); forward = oracle.grid2spec(grids) with
    nu_forward [17, 31]; rows[kcos] = oracle.spec2grid(spectra, kcos) with nu_rows[kcos] [17, 48]."""
    if "red" not in _cases:
        spectra = red_spectra(gold)
        grids = oracle.spec2grid_batch(spectra, 1)
        (forward,), (nu_forward,) = noise_floor(lambda g: (oracle.grid2spec_batch(g),), [grids], forward_bands)
        case = {"spectra": spectra, "grids": grids, "forward": forward, "nu_forward": nu_forward, "rows": {}, "nu_rows": {}}
        for kcos in (1, 2):
            (ref,), (nu,) = noise_floor(lambda s: (oracle.spec2grid_batch(s, kcos),), [spectra], row_errors)
            case["rows"][kcos], case["nu_rows"][kcos] = ref, nu
        assert np.array_equal(case["rows"][1], grids)
        _cases["red"] = case
    return _cases["red"]


OPERATORS = {"vort2vel": 2, "vel2vort": 2, "gradient": 1}  # name -> number of inputs; two outputs each
EXACT_OPERATORS = ("laplacian", "laplacian_inv", "truncate")  # one rounding per element


def operator_base():
    """(a, b): the first and the second input of base field i; b is a rotated by 7 fields."""
    a = seeded_spectra(N_BASE, triangular=False)
    return a, np.roll(a, -7, axis=0)


def operator_case(oracle):
    """dict name -> (reference outputs, nu per output [33, 32]) of the base fields, and name -> (reference,) for the exact ones."""
    if "ops" not in _cases:
        a, b = operator_base()
        case = {}
        for name, nin in OPERATORS.items():
            case[name] = noise_floor(oracle_operator(oracle, name), [a, b][:nin], spec_bands)
        for name in EXACT_OPERATORS:
            case[name] = oracle_operator(oracle, name)(a)
        _cases["ops"] = case
    return _cases["ops"]


def batch_factors(nfields):
    return 2.0 ** ((np.arange(nfields) // N_BASE) % 8 - 4)


def batch_of(base, nfields):
    """[33, ...] -> [nfields, ...]: field b = base[b % 33] * 2^((b // 33) % 8 - 4), for inputs and references alike."""
    f = batch_factors(nfields).reshape((nfields,) + (1,) * (base.ndim - 1))
    return base[np.arange(nfields) % N_BASE] * f
