"""CPU tier (oracle only): the conditions under which tests/test_transform_bands_gpu.py and tests/test_specops_gpu.py may hold the
device to clip(32 nu, 1e-13, 1e-11) per band and per latitude row (tests/transform_bands.py) -- the cap condition on the red
fields and on the operator inputs -- the exact scaling the batches are built on, and the demonstration that the band measure
rejects what the whole-field rule of tests/test_transforms_gpu.py lets through: ONE Legendre polynomial, (m, n) = (10, 18), off
by 1e-9 moves grid2spec of the temperature at the lowest level by 3.8e-14 of the field's maximum and band 28 by 33 times its
bound.  Figures: profiles/transform_bands.txt."""
import numpy as np
import pytest

import band_norms as bn
import transform_bands as tb


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir + "/step.npz")


def test_red_fields_are_red_and_fixed(oracle, gold):
    assert len(tb.RED_FIELDS) == 17 and len(set(tb.RED_FIELDS)) == 17
    case = tb.red_case(oracle, gold)
    assert case["spectra"].shape == (17, 32, 31) and case["grids"].shape == (17, 48, 96)
    ref = np.transpose(case["forward"], (2, 1, 0))  # (31, 32, 17)
    for f in range(17):
        mag = np.array([np.abs(ref[:, :, f][bn._L == l]).max() for l in range(31)])
        assert mag[30] < 1e-2 * mag.max(), (tb.red_name(f), mag[30] / mag.max())  # the tail is far below the field's maximum
    assert not case["forward"][:, 31, :].any()


def test_cap_condition_of_the_red_fields(oracle, gold):
    """32 nu of oracle.grid2spec <= CAP in every band 0 ... 30 of every red field (observed: at most 6.3e-13 in the humidity,
    5.8e-12 in the temperature)."""
    nu = tb.red_case(oracle, gold)["nu_forward"]
    assert nu.shape == (17, 31)
    for f in range(17):
        excess = bn.cap_excess(nu[f])
        print("%s: 32 nu of grid2spec %.2e" % (tb.red_name(f), excess))
        assert excess <= bn.CAP, (tb.red_name(f), excess)
    assert nu.max() > 0.0


@pytest.mark.parametrize("kcos", (1, 2))
def test_row_floor_of_the_red_fields(oracle, gold, kcos):
    """32 nu of oracle.spec2grid per latitude row <= CAP (observed: at most 1.3e-13)."""
    nu = tb.red_case(oracle, gold)["nu_rows"][kcos]
    assert nu.shape == (17, 48)
    for f in range(17):
        excess = bn.cap_excess(nu[f])
        print("%s, kcos %d: 32 nu of spec2grid per row %.2e" % (tb.red_name(f), kcos, excess))
        assert excess <= bn.CAP, (tb.red_name(f), kcos, excess)
    assert nu.min() > 0.0


@pytest.mark.parametrize("name", sorted(tb.OPERATORS))
def test_operator_floor(oracle, name):
    """32 nu per band <= CAP for the 33 base fields of the operator tests, band 31 (which has content here) included."""
    ref, nu = tb.operator_case(oracle)[name]
    for k in range(2):
        assert ref[k].shape == (33, 32, 31) and nu[k].shape == (33, 32) and np.isfinite(ref[k]).all()
        assert np.abs(ref[k][:, tb._BEYOND]).max() > 0 and np.abs(ref[k][:, 31, :]).max() > 0  # content beyond the truncation
        excess = bn.cap_excess(nu[k])
        print("%s output %d: 32 nu per band at most %.2e" % (name, k, excess))
        assert excess <= bn.CAP, (name, k, excess)


def test_operator_base_fields_fill_the_rectangle(oracle):
    a, b = tb.operator_base()
    assert a.shape == (33, 32, 31) and np.array_equal(b[0], a[7]) and np.array_equal(b[32], a[6])
    assert (np.abs(a) > 0).all() and not a[:, :, 0].imag.any()
    case = tb.operator_case(oracle)
    for name in tb.EXACT_OPERATORS:
        assert case[name][0].shape == (33, 32, 31) and np.isfinite(case[name][0]).all()
    x = tb.batch_of(a, 513)
    assert x.shape == (513, 32, 31)
    assert np.array_equal(x[0], a[0] * 2.0 ** -4) and np.array_equal(x[33], a[0] * 2.0 ** -3) and np.array_equal(x[512], a[17] * 2.0 ** 3)
    assert np.array_equal(x[8 * 33], x[0])  # the factors repeat after 264 fields ...
    assert len({x[i].tobytes() for i in range(264)}) == 264  # ... and no two fields before that are equal


def test_scaling_by_a_power_of_two_is_exact(oracle):
    """The batches of tests/test_specops_gpu.py rest on this: op(2^k a, 2^k b) == 2^k op(a, b) bitwise."""
    a, b = tb.operator_base()
    case = tb.operator_case(oracle)
    u, v = oracle.vort2vel(2.0 ** -3 * a[5].T, 2.0 ** -3 * b[5].T)
    assert np.array_equal(u.T, 2.0 ** -3 * case["vort2vel"][0][0][5]) and np.array_equal(v.T, 2.0 ** -3 * case["vort2vel"][0][1][5])
    for name, nin in tb.OPERATORS.items():
        for k in (-4, 3):
            got = tb.oracle_operator(oracle, name)(*[2.0 ** k * x[:3] for x in (a, b)[:nin]])
            for o in range(2):
                assert np.array_equal(got[o], 2.0 ** k * case[name][0][o][:3]), (name, k, o)
    for name in tb.EXACT_OPERATORS:
        assert np.array_equal(tb.oracle_operator(oracle, name)(8.0 * a[:3])[0], 8.0 * case[name][0][:3]), name


MUTATION = 1e-9


def test_band_bound_rejects_one_wrong_polynomial(oracle, gold):
    case = tb.red_case(oracle, gold)
    f = tb.RED_FIELDS.index(("t", 7, 1))
    grid, ref, nu = case["grids"][f:f + 1], case["forward"][f:f + 1], case["nu_forward"][f:f + 1]
    cpol = np.ctypeslib.as_array(oracle.tables().cpol).reshape((62, 32, 24), order="F")
    saved = cpol[20:22, 18, :].copy()
    try:
        cpol[20:22, 18, :] = saved * (1.0 + MUTATION)  # Re and Im rows of m = 10, n = 18, all latitudes
        wrong = oracle.grid2spec_batch(grid)
    finally:
        cpol[20:22, 18, :] = saved
    assert np.array_equal(oracle.grid2spec_batch(grid), ref)  # the table is back
    whole = tb.whole_fields(wrong, ref)[0]
    err = tb.forward_bands(wrong, ref)
    over = err > bn.bound(nu)
    print("one polynomial off by %.0e: whole field %.2e, %d of 31 bands over the bound, worst error / bound %.1f (l = %d)" % (
        MUTATION, whole, over.sum(), (err / bn.bound(nu)).max(), int((err / bn.bound(nu)).argmax())))
    assert whole <= tb.WHOLE_TOL  # the old rule lets it pass
    assert over.any()  # the band bound does not
    assert tb.forward_residue(wrong, ref)[0] <= tb.WHOLE_TOL and not wrong[:, 31, :].any()


def test_measures_on_hand_made_arrays():
    ref = np.zeros((2, 48, 96))
    ref[0] = np.arange(1, 49)[:, None]
    got = ref.copy()
    got[0, 3, 5] += 4e-3
    got[1, 7, 0] = 1e-5  # a field of zeros: the absolute error
    e = tb.row_errors(got, ref)
    assert e.shape == (2, 48) and e[0, 3] == pytest.approx(1e-3) and e[1, 7] == 1e-5 and np.count_nonzero(e) == 2
    s = np.zeros((1, 32, 31), dtype=np.complex128)
    s[0, 0, 0], s[0, 2, 3], s[0, 30, 1], s[0, 31, 30] = 100.0, 2.0, 0.5, 0.25  # l = 0, 5, 31 and the far corner
    g = s.copy()
    g[0, 2, 3] += 2e-6j
    g[0, 30, 1] += 1e-9
    assert np.allclose(tb.forward_bands(g, s)[0, [0, 5]], [0.0, 1e-6], rtol=1e-9) and tb.forward_bands(g, s).shape == (1, 31)
    assert tb.forward_residue(g, s)[0] == pytest.approx(1e-11) and tb.spec_bands(g, s)[0, 31] == pytest.approx(2e-9)
    assert tb.whole_fields(g, s)[0] == pytest.approx(2e-8)
