"""CPU tier: the index sets of csrc/triangle.hpp (through spd_get_table_host, no device) against the sets the reference's loops
define (tests/triangle_cases.py from legendre.f90:73, 150-161, 187, 206-217), and the amplitude of the halo-row content that
tests/test_triangle_gpu.py steps: admissible by the oracle alone (band_norms: MARGIN * nu <= CAP)."""
import ctypes as C

import numpy as np
import pytest

import band_norms as bn
import triangle_cases as tc


def host_table(hip_lib, name):
    n = hip_lib.spd_get_table_host(None, name.encode(), None, 0)
    assert n > 0, name
    buf = np.empty(n)
    assert hip_lib.spd_get_table_host(None, name.encode(), buf.ctypes.data_as(C.c_void_p), n) == n
    return buf


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir + "/step.npz")


def test_reference_sets_are_what_the_issue_counts():
    assert tc.INV_NEEDED.sum() == 527 and tc.FWD_FILLED.sum() == 526 and tc.HALO.sum() == 30
    assert np.array_equal(tc.INV_NEEDED, tc.L <= 31)
    assert [int(tc.FWD_FILLED[:, n].sum()) for n in range(32)] == [31, 31] + list(range(30, 1, -1)) + [0]
    assert not (tc.FWD_FILLED & ~tc.INV_NEEDED).any()


def test_nsh2_of_the_library_is_the_reference_rule(hip_lib):
    assert np.array_equal(host_table(hip_lib, "nsh2"), tc.NSH2)


def test_packed_index_is_a_bijection_in_row_order(hip_lib):
    t = host_table(hip_lib, "tri_packed")
    packed, index = int(t[0]), t[1:].reshape(32, 31).T  # [n][m] in the library -> (31 m, 32 n)
    assert np.array_equal(index, np.rint(index))
    index = index.astype(int)
    assert np.array_equal(index >= 0, tc.FWD_FILLED)
    # (n, m) order: row n behind the rows before it, m ascending inside a row
    order = [index[m, n] for n in range(32) for m in range(31) if tc.FWD_FILLED[m, n]]
    assert order == list(range(526))
    # whole 128-byte lines, and the arena's 256-byte carving holds for a packed complex128 field
    assert packed >= 526 and packed == 528 and packed * 16 % 256 == 0 and packed * 16 == 8448


def test_inverse_set_of_the_library(hip_lib):
    need = host_table(hip_lib, "tri_inv_needed").reshape(32, 31).T
    assert np.array_equal(need == 1.0, tc.INV_NEEDED) and np.array_equal(need == 0.0, ~tc.INV_NEEDED)


def test_halo_content_is_where_and_what_it_should_be(gold):
    base, halo = bn.perturbed_prognostics(gold, 2), tc.halo_prognostics(gold, 2)
    for n in bn.SPEC:
        changed = halo[n] != base[n]
        assert not changed[~tc.HALO].any() and np.isfinite(halo[n]).all()
        rms30 = np.sqrt((np.abs(base[n][tc.L == 30]) ** 2).mean(axis=0))
        rms32 = np.sqrt((np.abs(halo[n][tc.HALO]) ** 2).mean(axis=0))
        live = rms30 > 0
        assert live.any() and not rms32[~live].any()
        assert (rms32[live] > 0.5 * tc.HALO_FACTOR * rms30[live]).all() and (rms32[live] < 2.0 * tc.HALO_FACTOR * rms30[live]).all()
    assert not np.array_equal(tc.halo_prognostics(gold, 1)["t"][tc.HALO], halo["t"][tc.HALO])


def test_halo_amplitude_is_admissible(oracle, gold):
    """The rule of the issue: start at the rms of band 30, divide by 10 until the cap holds for every case; the factor it gives is
    the one the GPU tier uses (observed: factor 1 holds, worst MARGIN * nu 4.4e-12 against the cap 1e-11)."""
    factor = 1.0
    while True:
        worst = tc.worst_cap_excess(oracle, gold, factor)
        print("halo factor %g: worst MARGIN * nu %.2e (cap %.0e)" % (factor, worst, bn.CAP))
        if worst <= bn.CAP:
            break
        factor /= 10.0
        assert factor >= 1e-6, "no admissible amplitude"
    assert factor == tc.HALO_FACTOR, (factor, tc.HALO_FACTOR)
    # the halo row is in motion in the reference: it is carried forward, not zeroed
    ref, _ = tc.halo_case(oracle, gold, "startup", 0)
    assert all(np.abs(ref[-1][n][tc.HALO]).max() > 0 for n in bn.SPEC)


def test_the_halo_row_matters_to_the_reference(oracle, gold):
    """The GPU tier can only catch a mask that is one row too tight if the oracle's triangle depends on the halo row by more than
    the band bound (observed after the first call: vor, div change by more than their own size in 240 of 496 bands each)."""
    with_halo, _ = tc.halo_case(oracle, gold, "startup", 0)
    without, nu = bn.case(oracle, gold, "startup", 0)
    for n in ("vor", "div"):
        over = int((bn.band_errors(with_halo[0][n], without[0][n])[..., :31] > bn.bound(nu[0][n])[..., :31]).sum())
        assert over > 100, (n, over)
