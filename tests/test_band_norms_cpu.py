"""CPU tier (oracle only): the arithmetic of tests/band_norms.py on hand-made arrays; the cap condition for every case that
tests/test_step_bands_gpu.py holds the device to; and the demonstration that the band bound rejects what the whole-field norm
lets through -- the oracle stepped with dt-dependent tables (diffusion factors, implicit matrices, elz) built from
dt (1 + 1e-9) stays under the whole-field 1e-12 in t and tr after every call of the start-up sequence (observed 1.2e-14 ...
4.2e-13) and exceeds the band bound in 476 ... 480 of the 512 bands of t and 320 ... 332 of tr after it."""
import numpy as np
import pytest

import band_norms as bn


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir + "/step.npz")


def hand_made():
    """ref: level 0 holds m + n + 1 in every element inside the truncation; level 1 the same with band 5 zeroed; level 2 is zero."""
    l = np.add.outer(np.arange(31), np.arange(32))
    ref = np.zeros((31, 32, 3), dtype=np.complex128)
    ref[:, :, 0] = np.where(l <= 30, l + 1.0, 0.0)
    ref[:, :, 1] = np.where((l <= 30) & (l != 5), 2.0 * (l + 1.0), 0.0)
    return ref


def test_band_membership_and_own_scale():
    ref = hand_made()
    got = ref.copy()
    got[3, 4, 0] += 0.5j      # l = 7, level 0: scale 8
    got[0, 7, 0] -= 0.25      # the same band: the larger error counts
    got[30, 0, 0] += 31e-3    # l = 30, the last element of the last band inside the truncation
    got[0, 0, 1] += 1e-6      # l = 0, level 1: scale 2
    e = bn.band_errors(got, ref)
    assert e.shape == (3, 32)
    expect = np.zeros((3, 32))
    expect[0, 7], expect[0, 30], expect[1, 0] = 0.5 / 8.0, 1e-3, 0.5e-6
    assert np.allclose(e, expect, rtol=1e-9, atol=0.0)
    assert np.count_nonzero(e) == 3
    # the trailing shape is kept: (31, 32, 8, 2) -> (8, 2, 32), (31, 32, 2) -> (2, 32), (31, 32) -> (32,)
    assert bn.band_errors(np.zeros((31, 32, 8, 2)), np.zeros((31, 32, 8, 2))).shape == (8, 2, 32)
    assert bn.band_errors(got[:, :, :2], ref[:, :, :2]).shape == (2, 32)
    assert np.array_equal(bn.band_errors(got[:, :, 0], ref[:, :, 0]), e[0])


def test_scale_fall_backs():
    ref = hand_made()
    got = ref.copy()
    got[2, 3, 1] = 1e-3   # l = 5 of level 1: the band's reference is zero -> that level's maximum over all bands, 62
    got[1, 1, 2] = 1e-3   # level 2 is zero altogether -> the field's maximum, 62
    e = bn.band_errors(got, ref)
    assert e[1, 5] == pytest.approx(1e-3 / 62.0, rel=1e-12) and e[2, 2] == pytest.approx(1e-3 / 62.0, rel=1e-12)
    assert np.count_nonzero(e) == 2
    # a field of zeros: the absolute error
    z = np.zeros((31, 32), dtype=np.complex128)
    g = z.copy()
    g[0, 3] = 1e-5
    assert bn.band_errors(g, z)[3] == 1e-5


def test_beyond_the_truncation_is_exact():
    ref = hand_made()
    for m, n in ((0, 31), (30, 1), (15, 16), (30, 31), (20, 20)):  # l = 31 and the corner that no transform touches
        got = ref.copy()
        got[m, n, 1] = 1e-300
        e = bn.band_errors(got, ref)
        assert np.isinf(e[1, 31]) and np.count_nonzero(e) == 1, (m, n)
        assert not (e <= bn.bound(np.zeros_like(e))).all()
    assert not bn.band_errors(ref, ref).any()
    # a reference that is NOT zero there (the temperature: the imprint of tcorh) makes band 31 a band like the others
    ref[4, 27, 0] = 2e-5
    got = ref.copy()
    got[4, 27, 0] += 2e-17
    assert bn.band_errors(got, ref)[0, 31] == pytest.approx(1e-12, rel=1e-3)
    got[4, 27, 0] = 0.0
    assert bn.band_errors(got, ref)[0, 31] == 1.0


def test_bound_rule():
    nu = np.array([0.0, 3e-16, 1e-14, 1e-12])
    assert np.array_equal(bn.bound(nu), [1e-13, 1e-13, 32e-14, 1e-11])
    assert bn.cap_excess(nu) == 32e-12


def test_noise_floor_perturbs_every_prognostic_by_an_ulp():
    """run_oracle = the identity on the prognostics: nu is then the perturbation itself, at most 2^-52 (1 + 2^-52) in every
    band of every variable up to the product's own rounding, reached in most, and zero where the input is zero."""
    rng = np.random.default_rng(0)
    inputs = {n: (rng.standard_normal((31, 32, 2)) + 1j * rng.standard_normal((31, 32, 2))) * (bn._L <= 30)[:, :, None]
              for n in bn.SPEC}
    inputs["other"] = np.ones(3)
    seen = []

    def run(x):
        seen.append(x)
        return [{n: x[n] for n in bn.SPEC}]

    ref, nu = bn.noise_floor(run, inputs, 3)
    assert len(seen) == 4 and all(x["other"] is inputs["other"] for x in seen)
    for n in bn.SPEC:
        assert ref[0][n] is inputs[n]
        assert nu[0][n].shape == (2, 32) and nu[0][n].max() <= 2 * bn.ULP  # (the product rounds to one or two ulps of the element)
        assert (nu[0][n][:, 5:31] > 0).all() and np.median(nu[0][n][:, 5:31]) > 0.5 * bn.ULP and not nu[0][n][:, 31].any()
        for x in seen[1:]:
            assert not np.array_equal(x[n], inputs[n]) and np.abs(x[n] - inputs[n]).max() <= 2 * bn.ULP * np.abs(inputs[n]).max()
            assert np.array_equal(x[n] == 0, inputs[n] == 0)
    assert not np.array_equal(seen[1]["t"], seen[2]["t"])
    f = bn.ulp_factors(np.random.default_rng(3), (31, 32, 8, 2))
    assert f.dtype == np.float64 and set(np.unique(f)) == {1.0 - bn.ULP, 1.0, 1.0 + bn.ULP}


def test_cases_are_perturbed_as_stated(gold):
    a, b = bn.perturbed_prognostics(gold, 1), bn.perturbed_prognostics(gold, 2)
    for n in bn.SPEC:
        g = gold["s0_" + n]
        assert a[n].shape == g.shape and not a[n][0].imag.any()
        sel = g[1:] != 0
        r = (a[n][1:][sel] / g[1:][sel]).real - 1.0
        assert 0.9e-3 < r.std() < 1.1e-3 and abs(r.mean()) < 1e-4
        # the two time levels move independently, and so do the members
        r0, r1 = a[n][1:, ..., 0] / np.where(sel[..., 0], g[1:, ..., 0], 1), a[n][1:, ..., 1] / np.where(sel[..., 1], g[1:, ..., 1], 1)
        assert not np.array_equal(r0, r1) and not np.array_equal(a[n], b[n])


@pytest.mark.parametrize("sequence", sorted(bn.SEQUENCES))
def test_cap_condition_holds_for_every_case(oracle, gold, sequence):
    """MARGIN * nu <= CAP in every band, by the oracle alone, for the nine members the GPU tier steps (observed: worst nu
    2.3e-13, worst MARGIN * nu 7.2e-12); the reference is finite and in motion."""
    worst = 0.0
    for member in range(9):
        ref, nu = bn.case(oracle, gold, sequence, member)
        assert len(ref) == len(bn.SEQUENCES[sequence])
        for k in range(len(ref)):
            for n in bn.SPEC:
                assert np.isfinite(ref[k][n]).all() and np.abs(ref[k][n]).max() > 0
                excess = bn.cap_excess(nu[k][n])
                assert excess <= bn.CAP, (sequence, member, k, n, excess)
                worst = max(worst, excess)
    print("%s: worst MARGIN * nu %.2e (cap %.0e)" % (sequence, worst, bn.CAP))


@pytest.mark.parametrize("member", (1, 2))
def test_band_bound_rejects_tables_of_a_slightly_wrong_dt(oracle, gold, member):
    ref, nu = bn.case(oracle, gold, "startup", member)
    wrong = bn.sequence_runner(oracle, gold, "startup", lambda dt: dt * (1.0 + 1e-9))(bn.oracle_inputs(gold, member))
    for n in ("t", "tr"):
        for k in range(3):
            assert bn.whole_field(wrong[k][n], ref[k][n]) <= 1e-12, (n, k)  # what the older tests ask
        e = bn.band_errors(wrong[2][n], ref[2][n])
        over = int((e > bn.bound(nu[2][n])).sum())
        print("member %d, %s: whole field %.2e, %d of %d bands over the bound, worst band %.2e" %
              (member, n, bn.whole_field(wrong[2][n], ref[2][n]), over, e.size, e.max()))
        assert over > 100, (n, over)


def test_oracle_against_itself_is_zero(oracle, gold):
    ref, nu = bn.case(oracle, gold, "startup", 1)
    again = bn.sequence_runner(oracle, gold, "startup")(bn.oracle_inputs(gold, 1))
    for k in range(3):
        for n in bn.SPEC:
            e = bn.band_errors(again[k][n], ref[k][n])
            assert not e.any() and (e <= bn.bound(nu[k][n])).all(), (k, n)
