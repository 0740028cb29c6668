"""GPU tier: the device's transforms on RED fields -- humidity and temperature of the golden step state, whose spectra fall by
four orders of magnitude from l = 0 to l = 30 -- against the CPU oracle per total wavenumber (grid2spec, legendre) and per
latitude row (spec2grid, legendre_inv + fourier_inv), tests/transform_bands.py.  Every band 0 ... 30 and every row is held to
bound = clip(32 nu, 1e-13, 1e-11), nu from 4 one-ulp draws of the oracle's input (the cap condition is asserted by
tests/test_transform_bands_cpu.py, which also shows one wrong polynomial passing the whole-field rule and failing this one).
The elements with m + n >= 31 of a forward transform are quadrature residue and stay under the whole-field rule, 1e-13 of the
field's maximum; the column n = 31 is exactly zero.  Figures: profiles/transform_bands.txt.

legendre(fourier(x)) is NOT bitwise grid2spec(x), by design: the fused kernel forms (north row + south row) * weight and
(north row - south row) * weight of every latitude pair from the grid rows and transforms those (transforms.hip, grid2spec_body),
the stage calls -- like the reference -- transform the rows and combine the Fourier coefficients.  The FFT is linear, so the two
differ by roundings only; both are held to the same bound."""
import numpy as np
import pytest
import torch

import band_norms as bn
import transform_bands as tb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir + "/step.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def held(what, err, nu, unit, failures):
    """Print the worst error / bound of err, nu: [17, bands or rows], and note a failure (field f is RED_FIELDS[f])."""
    ratio, text = tb.report(err, nu, unit)
    print("%s: worst error / bound %.3f (%s)" % (what, ratio, text.splitlines()[0]))
    over = ~(err <= bn.bound(nu))
    if over.any():
        failures.append("%s: %d of %d over the bound; the worst (field f is transform_bands.RED_FIELDS[f]):\n%s" % (
            what, int(over.sum()), err.size, text))


def test_forward_transform_of_red_fields_per_band(spectral, oracle, gold):
    case = tb.red_case(oracle, gold)
    grids, ref, nu = dev(case["grids"]), case["forward"], case["nu_forward"]
    batched = spectral.grid2spec(grids)
    single = torch.stack([spectral.grid2spec(grids[f:f + 1])[0] for f in range(17)])
    staged = spectral.legendre(spectral.fourier(grids))
    failures = []
    for what, out in (("grid2spec", batched), ("legendre(fourier)", staged)):
        got = out.cpu().numpy()
        held("%s, 17 red fields" % what, tb.forward_bands(got, ref), nu, "l", failures)
        residue, whole = tb.forward_residue(got, ref), tb.whole_fields(got, ref)
        print("%s: worst residue beyond the truncation %.2e, worst whole-field figure %.2e" % (what, residue.max(), whole.max()))
        assert (residue <= tb.WHOLE_TOL).all() and (whole <= tb.WHOLE_TOL).all(), (what, residue.max(), whole.max())
        assert not got[:, 31, :].any(), what  # the column n = 31 is never filled
        assert not got[:, :, 0].imag.any(), what  # zonal-mean coefficients are real
    print("legendre(fourier(x)) bitwise grid2spec(x): %s" % torch.equal(staged, batched))
    assert torch.equal(single, batched)  # one launch per field: the same bits
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kcos", (1, 2))
def test_inverse_transform_of_red_fields_per_row(spectral, oracle, gold, kcos):
    case = tb.red_case(oracle, gold)
    spectra, ref, nu = dev(case["spectra"]), case["rows"][kcos], case["nu_rows"][kcos]
    fused = spectral.spec2grid(spectra, kcos)
    staged = spectral.fourier_inv(spectral.legendre_inv(spectra), kcos)
    single = torch.stack([spectral.spec2grid(spectra[f:f + 1], kcos)[0] for f in range(17)])
    failures = []
    for what, out in (("spec2grid", fused), ("fourier_inv(legendre_inv)", staged)):
        got = out.cpu().numpy()
        held("%s kcos %d, 17 red fields" % (what, kcos), tb.row_errors(got, ref), nu, "row", failures)
        whole = tb.whole_fields(got, ref)
        print("%s kcos %d: worst whole-field figure %.2e" % (what, kcos, whole.max()))
        assert (whole <= tb.WHOLE_TOL).all(), (what, whole.max())
    assert torch.equal(single, fused)
    assert not failures, "\n".join(failures)
