"""GPU tier: the spectral operators, the four stage calls and the two composite calls of ModSpectral on BATCHES, against one
oracle call per field (tests/transform_bands.py).

The operator kernels (csrc/specops.hip) run one thread per coefficient over a flat index of nfields * 992 in blocks of 256, so
blocks straddle fields; the table index is the flat index modulo 992 and the neighbours n - 1 / n + 1 lie 31 coefficients away,
in the previous or the next field for the rows n = 0 and n = 31 unless their branches are taken.  None of this shows at a batch
of one.  Batches: field b = base[b % 33] * 2^((b // 33) % 8 - 4) of 33 full-rectangle base fields, all fields distinct, the
reference scaled by the same exact factor.  vort2vel, vel2vort and gradient are held per total wavenumber to
clip(32 nu, 1e-13, 1e-11), band 31 (which has content here) included; laplacian, laplacian_inv and truncate are one rounding per
element and equal the oracle exactly.  The stage and composite calls are held to the whole-field rule of
tests/test_transforms_gpu.py, 1e-13 of every field's maximum.  Figures: profiles/transform_bands.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_norms as bn
import transform_bands as tb

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


@pytest.mark.parametrize("nfields", (1, 2, 8, 33, 513))
def test_operators_on_batches(spectral, oracle, nfields):
    """8 * 992 coefficients are a whole number of blocks; the other sizes end in a partial block."""
    case = tb.operator_case(oracle)
    base = tb.operator_base()
    host = [tb.batch_of(x, nfields) for x in base]
    ins = [dev(x) for x in host]
    pick = np.arange(nfields) % tb.N_BASE
    failures, worst = [], 0.0
    for name, nin in tb.OPERATORS.items():
        outs = getattr(spectral, name)(*ins[:nin])
        ref, nu = case[name]
        for k in range(2):
            got = outs[k].cpu().numpy()
            assert got.shape == (nfields, 32, 31)
            err, v = tb.spec_bands(got, tb.batch_of(ref[k], nfields)), nu[k][pick]
            ratio, text = tb.report(err, v)
            worst = max(worst, ratio)
            over = ~(err <= bn.bound(v))
            if over.any():
                failures.append("%s output %d, %d fields: %d of %d bands over the bound, in fields %s; the worst:\n%s" % (
                    name, k, nfields, int(over.sum()), err.size, np.flatnonzero(over.any(axis=1))[:12].tolist(), text))
    for name in ("laplacian", "laplacian_inv"):
        got = getattr(spectral, name)(ins[0]).cpu().numpy()
        want = tb.batch_of(case[name][0], nfields)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            failures.append("%s, %d fields: %d elements differ from the oracle, the first at [field, n, m] = %s" % (
                name, nfields, len(bad), bad[0].tolist()))
    for x, h in zip(ins, host):
        assert np.array_equal(x.cpu().numpy(), h)  # the out-of-place operators leave their inputs alone
    x = ins[0].clone()
    y = spectral.truncate(x)
    assert y is x  # in place, and returns its argument
    want = tb.batch_of(case["truncate"][0], nfields)
    if not np.array_equal(x.cpu().numpy(), want):
        bad = np.argwhere(x.cpu().numpy() != want)
        failures.append("truncate, %d fields: %d elements differ from the oracle, the first at [field, n, m] = %s" % (
            nfields, len(bad), bad[0].tolist()))
    print("operators, %d fields: worst error / bound %.3f" % (nfields, worst))
    assert not failures, "\n".join(failures)


def stage_inputs(nfields):
    """Seeded: full-rectangle spectra WITH an imaginary part in the zonal-mean coefficients (the reference's Legendre stage
    keeps it), white Fourier planes (their row 1, Im of m = 0, is not zero either) and white grids."""
    rng = np.random.default_rng(2024)
    ll = np.add.outer(np.arange(32), np.arange(31))
    spec = (rng.standard_normal((nfields, 32, 31)) + 1j * rng.standard_normal((nfields, 32, 31))) / (1.0 + ll)
    return spec, rng.standard_normal((nfields, 48, 62)), rng.standard_normal((nfields, 48, 96))


@pytest.mark.parametrize("nfields", (1, 3, 8, 65))
def test_stage_calls_on_batches(spectral, oracle, nfields):
    spec, four, grid = stage_inputs(nfields)
    assert np.abs(spec[:, :, 0].imag).min() > 0 and np.abs(four[:, :, 1]).min() > 0
    calls = (("legendre_inv", spec, ()), ("legendre", four, ()), ("fourier_inv", four, (1,)), ("fourier_inv", four, (2,)),
             ("fourier", grid, ()))
    worst = 0.0
    for name, x, args in calls:
        ref = tb.oracle_stage(oracle, name, x, *args)
        dx = dev(x)
        out = getattr(spectral, name)(dx, *args)
        whole = tb.whole_fields(out.cpu().numpy(), ref)
        worst = max(worst, whole.max())
        assert (whole <= tb.WHOLE_TOL).all(), "%s%r, %d fields: field %d at %.3e" % (name, args, nfields, whole.argmax(), whole.max())
        assert np.array_equal(dx.cpu().numpy(), x), name
        for b in range(nfields):  # field b of the batch is the one-field launch of field b, bit for bit
            assert torch.equal(getattr(spectral, name)(dx[b:b + 1], *args)[0], out[b]), (name, args, b)
    print("stage calls, %d fields: worst whole-field figure %.2e" % (nfields, worst))


def test_composite_calls_share_a_growing_scratch(oracle):
    """grid_vel2vort and grid_filter keep their spectral intermediates in one scratch buffer per handle (capi.hip: get_scratch).
    On a fresh handle: 2 fields (the buffer is made, then doubled), 9 (it grows twice more), 1 (it is larger than needed).
    Then spd_grid_filter with fg1 == fg2, as the model calls it."""
    import pyspeedy_amd
    from pyspeedy_amd._lib import check
    sp = pyspeedy_amd.ModSpectral()
    rng = np.random.default_rng(77)
    worst = 0.0
    for nfields in (2, 9, 1):
        ug, vg = rng.standard_normal((2, nfields, 48, 96))
        dug, dvg = dev(ug), dev(vg)
        filtered = sp.grid_filter(dug)
        ref = tb.per_field(oracle.grid_filter, 1, ug)[0]
        whole = tb.whole_fields(filtered.cpu().numpy(), ref)
        assert (whole <= tb.WHOLE_TOL).all(), ("grid_filter", nfields, whole.max())
        worst = max(worst, whole.max())
        for kcos in (1, 2):
            outs = sp.grid_vel2vort(dug, dvg, kcos)
            refs = tb.per_field(lambda u, v: oracle.grid_vel2vort(u, v, kcos), 2, ug, vg)
            for k in range(2):
                whole = tb.whole_fields(outs[k].cpu().numpy(), refs[k])
                assert (whole <= tb.WHOLE_TOL).all(), ("grid_vel2vort", kcos, k, nfields, whole.max())
                worst = max(worst, whole.max())
        assert np.array_equal(dug.cpu().numpy(), ug) and np.array_equal(dvg.cpu().numpy(), vg)
        p = dug.clone()
        ptr = C.c_void_p(p.data_ptr())
        check(sp._lib.spd_grid_filter(sp.handle, ptr, ptr, nfields, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "spd_grid_filter in place")
        assert torch.equal(p, filtered), nfields
    print("composite calls: worst whole-field figure %.2e" % worst)
    sp.close()


def test_empty_batches(spectral):
    g = torch.empty((0, 48, 96), dtype=torch.float64, device="cuda")
    s = torch.empty((0, 32, 31), dtype=torch.complex128, device="cuda")
    assert spectral.grid_filter(g).shape == (0, 48, 96)
    for kcos in (1, 2):
        assert [tuple(t.shape) for t in spectral.grid_vel2vort(g, g, kcos)] == [(0, 32, 31)] * 2
    for name, nin in tb.OPERATORS.items():
        assert [tuple(t.shape) for t in getattr(spectral, name)(*(s, s)[:nin])] == [(0, 32, 31)] * 2
    for name in ("laplacian", "laplacian_inv", "truncate"):
        assert getattr(spectral, name)(s).shape == (0, 32, 31)
    assert spectral.legendre_inv(s).shape == (0, 48, 62) and spectral.fourier(g).shape == (0, 48, 62)
    f = torch.empty((0, 48, 62), dtype=torch.float64, device="cuda")
    assert spectral.legendre(f).shape == (0, 32, 31) and spectral.fourier_inv(f, 2).shape == (0, 48, 96)
