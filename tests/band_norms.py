"""Helper of the band tests (not a test): errors of a spectral array per level, time level and total wavenumber, the oracle's own
rounding sensitivity in the same norm, and the states and call sequences that tests/test_band_norms_cpu.py (oracle only) and
tests/test_step_bands_gpu.py (device against oracle) share.

A whole-field figure max|got - ref| / max|ref| is blind wherever a field is small next to its maximum: the band l = 30 of the
temperature is 1.7e-5 of the mean-temperature coefficient, level 5 of the humidity 4.7e-3 of the lowest level.  Here every band
l = m + n of every level and time level is scaled by its own maximum, and the bound it is held to comes from the reference:
nu, the largest change of the oracle's result in that band when every prognostic input moves by at most one ulp, times a margin.

    bound = clip(MARGIN * nu, FLOOR, CAP)

MARGIN = 32: nu seeds ONE rounding per input; the device differs by one rounding at every contracted multiply-add along the chain
and by its exp / log inside the physics; five bits cover that.  FLOOR = 1e-13 is the tightest figure any kernel of this project
is held to (the transforms): it keeps bands whose nu is an ulp from demanding sub-ulp agreement.  CAP = 1e-11 is a condition on
the INPUTS, not a tolerance: they must be chosen so that MARGIN * nu stays under it by the oracle alone (cap_excess, asserted on
the CPU tier for every case the GPU tier uses)."""
import numpy as np

from test_step_oracle import DELT, STEP_2D

SPEC = ("vor", "div", "t", "tr", "ps")
MARGIN, FLOOR, CAP = 32.0, 1e-13, 1e-11
ULP = 2.0 ** -52

_L = np.add.outer(np.arange(31), np.arange(32))  # total wavenumber of element (m, n) of the registry layout
# [l][m]: position of element (m, l - m) in the flattened (31, 32) array, for l = 0 ... 30; 992 (a zero appended there) pads
_BAND_INDEX = np.array([[m * 32 + (l - m) if m <= l else 992 for m in range(31)] for l in range(31)])


def whole_field(got, ref):
    """The figure the older tests use: max|got - ref| / max|ref| over the whole array."""
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


def band_errors(got, ref):
    """got, ref: complex (31, 32[, 8][, 2]) -> float array [trailing shape..., 32]: for every trailing index (level, time level)
    and every total wavenumber l = m + n, max|got - ref| over the band / scale, where scale is the band's own max|ref|, or if
    that is exactly zero the maximum of that level and time level over all bands, or if that is zero too the field's maximum
    (and 1 for a field of zeros, so that the figure is then the absolute error).

    Band 31 lies beyond the truncation (trfilt = 0; the elements with m + n > 31, which no transform touches, are counted with
    it).  Where the reference is exactly zero there -- everywhere but in the temperature -- the comparison is exact: 0.0 when got
    is exactly zero in all of it, inf otherwise, which no bound admits.  The temperature is the exception: the reference state
    carries the imprint of the orographic correction tcorh in l = 31 (1.7e-5 K in the golden state; no tendency ever reaches it,
    only the Robert filter mixes its two time levels), so a device that zeroed it would be wrong; a band 31 in which the
    reference is not zero is a band like any other, scaled by its own maximum."""
    got, ref = np.asarray(got, dtype=np.complex128), np.asarray(ref, dtype=np.complex128)
    assert got.shape == ref.shape and got.shape[:2] == (31, 32), (got.shape, ref.shape)
    trailing = got.shape[2:]
    g, r = got.reshape(31, 32, -1), ref.reshape(31, 32, -1)
    J = g.shape[2]
    zero = np.zeros((1, J))
    diff = np.concatenate([np.abs(g - r).reshape(992, J), zero])[_BAND_INDEX].max(axis=1)  # [31 bands][J]
    mag = np.concatenate([np.abs(r).reshape(992, J), zero])[_BAND_INDEX].max(axis=1)
    slab = mag.max(axis=0, keepdims=True)  # per level and time level, over the bands inside the truncation
    field = slab.max()
    scale = np.where(mag > 0.0, mag, np.where(slab > 0.0, slab, field if field > 0.0 else 1.0))
    out = np.empty((J, 32))
    out[:, :31] = (diff / scale).T
    beyond = _L.reshape(992) >= 31
    g31, r31 = np.abs(g.reshape(992, J)[beyond]).max(axis=0), np.abs(r.reshape(992, J)[beyond]).max(axis=0)
    d31 = np.abs(g - r).reshape(992, J)[beyond].max(axis=0)
    out[:, 31] = np.where(r31 > 0.0, d31 / np.where(r31 > 0.0, r31, 1.0), np.where(g31 > 0.0, np.inf, 0.0))
    return out.reshape(trailing + (32,))


def ulp_factors(rng, shape):
    """1 + 2^-52 * r with r in {-1, 0, 1} per element (real: a zero imaginary part stays zero)."""
    return 1.0 + ULP * rng.integers(-1, 2, size=shape).astype(np.float64)


def noise_floor(run_oracle, inputs, draws):
    """The reference's own rounding sensitivity nu.  run_oracle(inputs) -> list (one entry per call) of dicts name -> spectral
    array; inputs: dict that holds the prognostic arrays SPEC (both time levels) among whatever else run_oracle needs.
    -> (reference, nu): the result for the inputs as they are, and per call and name the largest band_errors between it and
    `draws` results, in each of which every element of every prognostic input is multiplied by ulp_factors from
    default_rng(draw).  Only the oracle runs here."""
    reference = run_oracle(inputs)
    nu = [{n: np.zeros(a.shape[2:] + (32,)) for n, a in call.items()} for call in reference]
    for draw in range(draws):
        rng = np.random.default_rng(draw)
        moved = dict(inputs)
        for n in SPEC:
            moved[n] = inputs[n] * ulp_factors(rng, inputs[n].shape)
        for k, call in enumerate(run_oracle(moved)):
            for n, a in call.items():
                nu[k][n] = np.maximum(nu[k][n], band_errors(a, reference[k][n]))
    return reference, nu


def bound(nu):
    return np.clip(MARGIN * nu, FLOOR, CAP)


def cap_excess(nu):
    """Largest MARGIN * nu over the bands: the inputs are admissible when this is <= CAP."""
    return MARGIN * float(np.max(nu))


def worst_bands(err, nu, count=10):
    """[(trailing index..., l, error, nu, bound)] of the `count` bands with the largest error / bound, worst first."""
    b = bound(nu)
    ratio = err / b
    order = np.argsort(ratio, axis=None)[::-1][:count]
    rows = []
    for flat in order:
        idx = np.unravel_index(flat, err.shape)
        rows.append(tuple(int(i) for i in idx) + (float(err[idx]), float(nu[idx]), float(b[idx])))
    return rows


def describe(rows, trailing_names):
    """worst_bands rows as text: 'level 3, time level 1, l 30: error 2.1e-12, nu 3.0e-15, bound 1.0e-13'."""
    lines = []
    for row in rows:
        idx, (l, e, v, b) = row[:-4], row[-4:]
        where = ", ".join("%s %d" % (name, i) for name, i in zip(trailing_names, idx))
        lines.append("%sl %d: error %.3e, nu %.3e, bound %.3e" % (where + ", " if where else "", l, e, v, b))
    return "\n".join(lines)


def trailing_names(name):
    return ("time level",) if name == "ps" else ("level", "time level")


# ---- the cases: perturbed golden step states and the call sequences run on them ------------------------------------------------
# (j1, j2, dt, compute_shortwave) per call; the dt-dependent tables are rebuilt for `dt` before every call
SEQUENCES = {
    # time_stepping.f90:13-27 (first_step) on a state in motion: forward half step, forward step, leapfrog
    "startup": ((1, 1, 0.5 * DELT, True), (1, 2, DELT, False), (2, 2, 2 * DELT, False)),
    # leapfrog at a step length other than the 2 DELT every other test builds its tables for
    "leapfrog_delt": ((2, 2, DELT, True), (2, 2, DELT, False)),
}
NOISE_DRAWS = 4


def perturbed_prognostics(gold, member):
    """The golden state before step 42 with every prognostic, both time levels independently, multiplied by 1 + 1e-3 N(0, 1)
    from default_rng(member); the zonal-mean coefficients keep a zero imaginary part."""
    rng = np.random.default_rng(member)
    out = {}
    for n in SPEC:
        a = gold["s0_" + n] * (1.0 + 1e-3 * rng.standard_normal(gold["s0_" + n].shape))
        a[0] = a[0].real
        out[n] = a
    return out


def oracle_inputs(gold, member):
    arr = {n: gold["s0_" + n] for n in ("phis",) + STEP_2D}
    arr.update(perturbed_prognostics(gold, member))
    arr["tcorh"], arr["qcorh"] = gold["tab_tcorh"], gold["tab_qcorh"]
    return arr


def sequence_runner(oracle, gold, sequence, table_dt=lambda dt: dt):
    """run_oracle for noise_floor: the calls of SEQUENCES[sequence] on a fresh oracle.ModelState, the state after every call.
    table_dt maps a call's dt to the dt its tables are built from (the identity, except to make the tables subtly wrong)."""
    def run(inputs):
        st = oracle.ModelState(inputs, True, float(gold["air_absortivity_co2"]))
        calls = []
        for j1, j2, dt, shortwave in SEQUENCES[sequence]:
            st.set_shortwave(shortwave)
            oracle.step(st, oracle.dyn_tables(table_dt(dt)), j1, j2, dt)
            calls.append({n: st.a[n].copy() for n in SPEC})
        return calls
    return run


_cases = {}


def case(oracle, gold, sequence, member):
    """(reference, nu) of one member and sequence, computed once per session and shared: treat both as read-only."""
    key = (sequence, member)
    if key not in _cases:
        _cases[key] = noise_floor(sequence_runner(oracle, gold, sequence), oracle_inputs(gold, member), NOISE_DRAWS)
    return _cases[key]
