"""Helper of the triangle tests (not a test): the index sets of the triangular truncation as the reference defines them, and the
step states with content in the halo row m + n = 32 that tests/test_triangle_cpu.py (oracle only: is the input admissible?)
and tests/test_triangle_gpu.py (device against oracle) share.

Registry layout of a spectral array: complex (31 m, 32 n[, 8 levels][, 2 time levels]).

The halo row: the inverse transforms read a spectral field only where m + n <= 31 (nsh2, legendre.f90:73, 150-161), but u and v are
formed from vorticity and divergence with an n +- 1 stencil (spectral.f90:190-214), so ucos / vcos at m + n = 31 use the state at
m + n = 32.  A kernel that skips coefficients by a mask that is one row too tight loses that term and nothing else; the golden
state is zero there, so no other test would notice."""
import numpy as np

import band_norms as bn

_M, _N = np.meshgrid(np.arange(31), np.arange(32), indexing="ij")  # (31, 32): m, n of the registry layout
L = _M + _N

# legendre.f90:68-77: nsh2(n) = 2 * #{m : m + n <= trunc + 1} real slots per row, trunc = 30 (0-based m, n here)
NSH2 = np.array([2 * int(((np.arange(31) + n) <= 31).sum()) for n in range(32)])
# legendre.f90:150-161: the inverse transform reads input(1 : nsh2(n), n) of every row
INV_NEEDED = _M < (NSH2 // 2)[None, :]
# legendre.f90:187, 206-217: the direct transform zeroes the output and fills rows n = 1 ... trunc + 1 (1-based), 1 : nsh2(n) of each
FWD_FILLED = INV_NEEDED & (_N <= 30)
HALO = L == 32

# Amplitude of the halo content relative to the rms of band 30 of the same variable, level and time level.  Found by
# tests/test_triangle_cpu.py::test_halo_amplitude_is_admissible with the rule: start at 1, divide by 10 until MARGIN * nu <= CAP
# holds by the oracle alone for every member, sequence, call and variable the GPU tier uses.  That test fails if the rule no
# longer gives this figure.
HALO_FACTOR = 1.0
HALO_MEMBERS = 9
_HALO_SEED = 3200


def halo_prognostics(gold, member, factor=None):
    """bn.perturbed_prognostics(gold, member) with content at exactly m + n = 32 in every prognostic, level and time level:
    factor * rms(band 30 of that variable, level, time level) * (N(0, 1) + i N(0, 1)) / sqrt(2), default_rng(3200 + member)."""
    factor = HALO_FACTOR if factor is None else factor
    rng = np.random.default_rng(_HALO_SEED + member)
    out = {}
    for n, a in bn.perturbed_prognostics(gold, member).items():
        a = a.copy()
        rms30 = np.sqrt((np.abs(a[L == 30]) ** 2).mean(axis=0))  # [trailing shape]
        assert rms30.max() > 0, n  # (zero where the field is: the humidity of the upper levels)
        shape = (int(HALO.sum()),) + a.shape[2:]
        z = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
        assert not a[HALO].any()  # the golden state is empty there
        a[HALO] = factor * rms30 * z
        out[n] = a
    return out


def halo_inputs(gold, member, factor=None):
    arr = bn.oracle_inputs(gold, member)
    arr.update(halo_prognostics(gold, member, factor))
    return arr


_cases = {}


def halo_case(oracle, gold, sequence, member, factor=None):
    """(reference, nu) of bn.noise_floor for one member and sequence on the halo inputs; computed once per session, read-only."""
    factor = HALO_FACTOR if factor is None else factor
    key = (sequence, member, factor)
    if key not in _cases:
        _cases[key] = bn.noise_floor(bn.sequence_runner(oracle, gold, sequence), halo_inputs(gold, member, factor), bn.NOISE_DRAWS)
    return _cases[key]


def worst_cap_excess(oracle, gold, factor):
    """Largest MARGIN * nu over every member, sequence, call and variable of the halo cases at this amplitude."""
    worst = 0.0
    for sequence in sorted(bn.SEQUENCES):
        for member in range(HALO_MEMBERS):
            ref, nu = halo_case(oracle, gold, sequence, member, factor)
            for k in range(len(ref)):
                for n in bn.SPEC:
                    assert np.isfinite(ref[k][n]).all()
                    worst = max(worst, bn.cap_excess(nu[k][n]))
    return worst
