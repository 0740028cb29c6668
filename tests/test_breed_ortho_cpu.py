"""CPU tier: orthonormalised breeding.  The arbiter (tests/breed_ortho_reference.py, written from the
definition) against the host compile of the device's factor routine (spd_breed_factor_host), bit for bit; the arbiter on its own
against numpy's QR; its Gram diagonal against the breeding arbiter's energies; the family check; the entry points are declared,
exported and bound; calls on a null model; the example parses its arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import breed_ortho_reference as ortho
import breed_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORTHO_SYMBOLS = ("spd_model_breed_orthogonalize", "spd_model_breed_gram", "spd_breed_family_check", "spd_breed_factor_host",
                 "spd_model_breed_ortho_info")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def factor_host(hip_lib, g, target):
    g = np.ascontiguousarray(g, dtype=np.float64)
    r = len(g)
    rdiag, coef, rank = np.full(r, -7.0), np.full((r, r), -7.0), C.c_int(-7)
    as_double = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rc = hip_lib.spd_breed_factor_host(as_double(g), r, float(target), as_double(rdiag), as_double(coef), C.byref(rank))
    assert rc == 0, hip_lib.spd_last_error()
    return rdiag, coef, rank.value


def spd_gram(rng, r, columns=200):
    a = rng.standard_normal((r, columns)) * rng.uniform(0.1, 10.0, (r, 1))
    return a @ a.T


# ---- the factor routine: arbiter against the library, bit for bit -------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2, 3, 19, 64])
def test_factor_of_the_library_is_the_arbiters_bit_for_bit(hip_lib, r):
    rng = np.random.default_rng(r)
    g, target = spd_gram(rng, r), 0.37
    R, c, rank = ortho.factor(g, target)
    rdiag, coef, got_rank = factor_host(hip_lib, g, target)
    assert rank == got_rank == r
    assert (np.diag(R) > 0).all() and np.array_equal(bits(rdiag), bits(np.diag(R)))
    assert np.array_equal(bits(coef), bits(c)), int((bits(coef) != bits(c)).sum())
    assert not np.tril(coef, -1).any() and coef[np.triu_indices(r)].all()
    # (the arbiter is a factorisation: R^T R = G and C = target R^-1 to rounding -- Cholesky's backward error, r 2^-53 |G|)
    assert np.abs(R.T @ R - g).max() <= 4 * r * 2.0 ** -53 * np.abs(g).max()
    assert np.abs(R @ c / target - np.eye(r)).max() < 1e-8


def test_factor_breaks_at_a_duplicated_vector(hip_lib):
    """Small integers, so that every operation is exact: v = (2, 0, 0), (1, 3, 0), (2, 0, 0) again, (1, 1, 1).  R_11 = 2, R_12 = 1,
    R_22 = 3, R_13 = 2, R_23 = 0 and the third radicand is 4 - 4 - 0 = 0: the family breaks at the duplicate."""
    v = np.array([[2.0, 0, 0], [1, 3, 0], [2, 0, 0], [1, 1, 1]])
    g = v @ v.T
    R, c, rank = ortho.factor(g, 6.0)
    assert rank == 2 and np.diag(R).tolist() == [2.0, 3.0, 0.0, 0.0] and R[0, 1] == 1.0
    assert c[:2, :2].tolist() == [[3.0, -1.0], [0.0, 2.0]] and not c[2:].any() and not c[:, 2:].any()
    rdiag, coef, got_rank = factor_host(hip_lib, g, 6.0)
    assert got_rank == 2 and np.array_equal(bits(rdiag), bits(np.diag(R))) and np.array_equal(bits(coef), bits(c))


def test_factor_breaks_at_a_nan_and_at_what_is_not_positive(hip_lib):
    g = spd_gram(np.random.default_rng(5), 5)
    g[1, 3] = g[3, 1] = np.nan  # (R_24 is NaN, so the fourth radicand is)
    R, c, rank = ortho.factor(g, 2.0)
    rdiag, coef, got_rank = factor_host(hip_lib, g, 2.0)
    assert rank == got_rank == 3
    assert np.array_equal(bits(rdiag), bits(np.diag(R))) and np.array_equal(bits(coef), bits(c)) and np.isfinite(coef).all()
    for first in (0.0, -1.0, np.inf, np.nan):  # the first member has nothing, or nothing finite: nobody is transformed
        g = spd_gram(np.random.default_rng(6), 3)
        g[0, 0] = first
        assert ortho.factor(g, 2.0)[2] == 0
        rdiag, coef, got_rank = factor_host(hip_lib, g, 2.0)
        assert got_rank == 0 and not rdiag.any() and not coef.any()


def test_factor_host_checks_its_arguments(hip_lib):
    one = (C.c_double * 1)(1.0)
    rank = C.c_int()
    assert hip_lib.spd_breed_factor_host(one, 0, 1.0, one, one, C.byref(rank)) == -1
    assert b"spd_breed_factor_host: r must be 1 ... 64, got 0" in hip_lib.spd_last_error()
    assert hip_lib.spd_breed_factor_host(one, 65, 1.0, one, one, C.byref(rank)) == -1
    assert hip_lib.spd_breed_factor_host(None, 1, 1.0, one, one, C.byref(rank)) == -1
    assert b"spd_breed_factor_host: null argument" in hip_lib.spd_last_error()


# ---- the arbiter on its own -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def family(golden_dir):
    """Five members around the golden state of day 1: its difference to day 3, every coefficient scaled by its own N(1, 0.5)"""
    run = np.load(os.path.join(golden_dir, "run.npz"))
    elm2 = np.load(os.path.join(golden_dir, "tables.npz"))["elm2"]
    xc = {n: run["d1_" + n] for n in ref.NAMES}
    rng = np.random.default_rng(11)
    members = []
    for _ in range(5):
        members.append({n: xc[n] + (run["d3_" + n] - xc[n]) * (1.0 + 0.5 * rng.standard_normal(xc[n].shape)) for n in ref.NAMES})
    weights = {n: np.linspace(0.5, 2.0, 8) for n in ref.NAMES}
    return members, xc, weights, elm2


def test_arbiter_is_a_qr_of_the_weighted_vectors(family):
    """Independent of the library.  V: the members' weighted real vectors as columns, G = V^T V.  numpy's Householder QR of V with
    the signs fixed gives R; the arbiter's R from G (CholeskyQR) and the orthonormality of V C / target -- the arbiter's own
    combination of the differences, in the weighted space -- are held to 64 r kappa(G) 2^-53, CholeskyQR's error form, in the
    spectral norm, relative.  Observed: R 1.4e-16, orthonormality 8.8e-16 against a bound of 1.2e-12 (kappa(G) = 32.5)."""
    members, xc, weights, elm2 = family
    r, target = len(members), 3.0
    v = np.stack([ortho.weighted_vector(x, xc, weights, elm2) for x in members], axis=1)
    g, _ = ortho.gram(members, xc, weights, elm2)
    assert np.abs(v.T @ v - g).max() <= 1e-12 * np.abs(g).max()  # (the same inner product, summed two ways)
    R, c, rank = ortho.factor(g, target)
    assert rank == r
    q, rq = np.linalg.qr(v)
    sign = np.sign(np.diag(rq))
    rq = sign[:, None] * rq
    bound = 64 * r * np.linalg.cond(g) * 2.0 ** -53
    err_r = np.linalg.norm(R - rq, 2) / np.linalg.norm(rq, 2)
    new = np.stack([ortho.combine([v[:, i] for i in range(r)], c, j) for j in range(r)], axis=1)
    err_q = np.linalg.norm(new.T @ new / target ** 2 - np.eye(r), 2)
    print("kappa(G) = %.3g, bound %.2e: R against QR %.2e, orthonormality %.2e" % (np.linalg.cond(g), bound, err_r, err_q))
    assert err_r <= bound and err_q <= bound, (err_r, err_q, bound)
    # ... and the transform on the states is that combination: the new members' Gram matrix is target^2 I up to the rounding of
    # X_c + acc, 2^-53 |X_c| per coefficient against perturbations of a few percent of it (1e-12 is far above both)
    moved = ortho.transform(members, xc, c, rank)
    g2, _ = ortho.gram(moved, xc, weights, elm2)
    assert np.abs(g2 / target ** 2 - np.eye(r)).max() < 1e-12
    for x, y in zip(members, moved):  # m + n >= 32 is not touched
        assert all(np.array_equal(x[n][~ref.INSIDE], y[n][~ref.INSIDE]) and not np.array_equal(x[n], y[n]) for n in ref.NAMES)


def test_arbiter_gram_diagonal_is_the_breeding_arbiters_energy(family):
    members, xc, weights, elm2 = family
    g, s = ortho.gram(members, xc, weights, elm2)
    assert np.array_equal(g, g.T) and np.array_equal(np.diag(g), np.diag(s))  # (the diagonal's terms are not negative)
    for j, x in enumerate(members):
        e = ref.energies(x, xc, elm2)
        want = sum(float((weights[n][:len(e[n])] * e[n]).sum()) for n in ref.NAMES)
        assert abs(g[j, j] / want - 1.0) < 1e-12, (j, g[j, j], want)
        assert abs(np.sqrt(g[j, j]) / ref.amplitude(x, xc, weights, elm2) - 1.0) < 1e-12
    # a family of one: the transform is plain breeding's rescale, bit for bit
    R, c, rank = ortho.factor(g[:1, :1], 0.5)
    s0 = np.float64(0.5) / np.sqrt(np.float64(g[0, 0]))
    assert rank == 1 and bits(c[0, 0]) == bits(s0)
    mine, plain = ortho.transform(members[:1], xc, c, 1)[0], ref.rescale(members[0], xc, s0)
    assert all(np.array_equal(bits(mine[n].view(np.float64)), bits(plain[n].view(np.float64))) for n in ref.NAMES)


# ---- the family check -------------------------------------------------------------------------------------------------------------
def family_check(hip_lib, control):
    ctl = np.asarray(control, dtype=np.int32)
    return hip_lib.spd_breed_family_check(ctl.ctypes.data_as(C.POINTER(C.c_int32)), len(ctl)), hip_lib.spd_last_error()


def test_family_check(hip_lib):
    assert family_check(hip_lib, [-1] + [0] * 64)[0] == 64
    rc, text = family_check(hip_lib, [-1] + [0] * 65)
    assert rc == -1 and b"spd_model_breed_orthogonalize: the family of control 0 has 65 members: at most 64 can be orthogonalised" in text
    rc, text = family_check(hip_lib, [1] + [-1] + [1] * 70 + [-1] + [72] * 3)
    assert rc == -1 and b"the family of control 1 has 71 members" in text
    assert family_check(hip_lib, [-1, 0, 0, 0, 7, 7, 7, -1])[0] == 3
    assert family_check(hip_lib, [-1, 0, 0, 0, 7, -1, -1, -1])[0] == 3
    assert family_check(hip_lib, [-1, -1])[0] == 0
    for control, message in (([-1, 0, 1], b"the control of member 2 (1) is itself bred: a control must have -1 (no chains)"),
                             ([-1, 1, 0], b"member 1 is its own control"),
                             ([-1, 0, 3], b"the control of member 2 (3) is out of range (-1 ... 2)"),
                             ([-1, -2, 0], b"the control of member 1 (-2) is out of range")):
        rc, text = family_check(hip_lib, control)
        assert rc == -1 and message in text, text
    assert hip_lib.spd_breed_family_check(None, 3) == -1 and b"spd_breed_family_check: null control" in hip_lib.spd_last_error()


# ---- the symbols, the null model, the example ----------------------------------------------------------------------------------
def test_ortho_symbols_declared_exported_and_bound(hip_lib):
    import inspect

    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in ORTHO_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for method in ("breed_orthogonalize", "breed_gram", "breed_exponents"):
        assert hasattr(EnsembleModel, method), method
    configure = inspect.signature(EnsembleModel.breed_configure).parameters
    assert configure["orthogonalize"].default is False and list(configure)[-1] == "orthogonalize"  # (existing calls are unchanged)
    assert inspect.signature(EnsembleModel.breed_orthogonalize).parameters["on"].default is True
    assert inspect.signature(EnsembleModel.breed_exponents).parameters["skip"].default == 1


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    n = C.c_int()
    assert hip_lib.spd_model_breed_orthogonalize(None, 1) == -1
    assert b"spd_model_breed_orthogonalize: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_breed_gram(None, None, 0, None) == -1 and b"spd_model_breed_gram: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_breed_ortho_info(None, C.byref(n), None, None) == -1
    assert b"spd_model_breed_ortho_info: null model" in hip_lib.spd_last_error()


def test_exponents_are_the_time_mean_of_the_growth_rates():
    """breed_exponents is host arithmetic on breed_growth(): checked on a stand-in that supplies the growth rates"""
    from pyspeedy_amd.model import EnsembleModel

    class Stub:
        def breed_growth(self):
            g = np.full((4, 3), np.nan)  # member 0 is not bred; the first event has no rate
            g[1:, 1] = [1e-6, 2e-6, 3e-6]
            g[1:, 2] = [5e-6, np.nan, -1e-6]
            return g

    got = EnsembleModel.breed_exponents(Stub())
    assert np.isnan(got[0]) and np.allclose(got[1:], [86400 * 2e-6, 86400 * 2e-6], rtol=1e-15)
    assert np.allclose(EnsembleModel.breed_exponents(Stub(), skip=2)[1:], [86400 * 2.5e-6, 86400 * -1e-6], rtol=1e-15)


def test_lyapunov_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("lyapunov_spectrum", os.path.join(ROOT, "examples", "lyapunov_spectrum.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.days, args.every, args.norm, args.noise) == (8, 30, 9, "total_energy", 0.01)
    args = mod.parse(["--members", "64", "--days", "60", "--every", "36", "--norm", "kinetic_energy", "--noise", "0.1"])
    assert (args.members, args.days, args.every, args.norm, args.noise) == (64, 60, 36, "kinetic_energy", 0.1)
    assert mod.control_of(4).tolist() == [-1, 0, 0, 0]
    assert mod.dimension(np.diag([2.0, 2.0, 2.0])) == pytest.approx(3.0) and mod.dimension(np.ones((3, 3))) == pytest.approx(1.0)
    for bad in (["--members", "1"], ["--members", "66"], ["--every", "0"], ["--norm", "enstrophy"]):
        with pytest.raises(SystemExit):
            mod.parse(bad)
