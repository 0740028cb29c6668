"""CPU tier: the assimilation.  The arbiter (tests/assim_reference.py, written from the definition) against the
host compile of the device's weights routine (spd_assim_weights_host), bit for bit; the arbiter on its own against the textbook
batch Kalman update in observation space; the argument checks without a model (spd_assim_check, the observation table); the entry
points are declared, exported and bound; calls on a null model; the example parses its arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import assim_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSIM_SYMBOLS = ("spd_model_assim_configure", "spd_model_assim_set_observations", "spd_model_assim_apply", "spd_model_assim_compute",
                 "spd_model_assim_transform", "spd_model_assim_read", "spd_model_assim_rows", "spd_model_assim_weights",
                 "spd_model_assim_info", "spd_model_assim_reset", "spd_model_assim_off", "spd_assim_check", "spd_assim_weights_host")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def as_double(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def weights_host(hip_lib, Y, yo, R, rho):
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    yo, R = np.ascontiguousarray(yo, dtype=np.float64), np.ascontiguousarray(R, dtype=np.float64)
    E, r = Y.shape
    W, stats = np.full((r, r), -7.0), np.full((E, 4), -7.0)
    rc = hip_lib.spd_assim_weights_host(as_double(Y), E, r, as_double(yo), as_double(R), float(rho), as_double(W), as_double(stats))
    assert rc == 0, hip_lib.spd_last_error()
    return W, stats


def seeded(r, E, seed):
    """rows of different means and spreads, observations within a few standard deviations, variances of the spreads' size"""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.1, 10.0, (E, 1))
    Y = rng.uniform(-50.0, 300.0, (E, 1)) + scale * rng.standard_normal((E, r))
    yo = Y.mean(axis=1) + scale[:, 0] * rng.standard_normal(E)
    R = scale[:, 0] ** 2 * rng.uniform(0.25, 4.0, E)
    return Y, yo, R


# ---- the weights routine: arbiter against the library, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("special", ["plain", "nan", "constant"])
@pytest.mark.parametrize("rho", [1.0, 1.1])
@pytest.mark.parametrize("r,E", [(2, 1), (3, 5), (19, 64), (64, 64)])
def test_weights_of_the_library_are_the_arbiters_bit_for_bit(hip_lib, r, E, rho, special):
    """`nan`: the observation of entry E // 2 is missing.  `constant`: the Y row of entry E // 2 is constant -- at 0.0, the one
    constant whose y_j = sum_i Y_i W_ij are equal whatever rounding W's column sums carry (the all-zero weight map of the GPU
    tier), so s = 0 exactly and the entry must be unused."""
    Y, yo, R = seeded(r, E, 1000 * r + E)
    k = E // 2
    if special == "nan":
        yo[k] = np.nan
    if special == "constant":
        Y[k] = 0.0
    W, stats = ref.weights(Y, yo, R, rho)
    got_W, got_stats = weights_host(hip_lib, Y, yo, R, rho)
    assert np.isfinite(W).all() and np.isfinite(stats).all()
    assert np.array_equal(bits(got_W), bits(W)), int((bits(got_W) != bits(W)).sum())
    assert np.array_equal(bits(got_stats), bits(stats)), int((bits(got_stats) != bits(stats)).sum())
    used = np.ones(E)
    if special != "plain":
        used[k] = 0.0
    assert stats[:, 3].tolist() == used.tolist()
    if special == "nan":
        assert stats[k, 2] == 0.0 and stats[k, 1] > 0.0
    if special == "constant":
        assert stats[k, 0] == 0.0 and stats[k, 1] == 0.0 and bits(stats[k, 2]) == bits(yo[k])
    start = np.full((r, r), (1.0 - rho) / r)
    np.fill_diagonal(start, (1.0 - rho) / r + rho)
    assert np.array_equal(W, start) == (not used.any())  # (a used entry moves W; none leaves the inflation matrix)


@pytest.mark.parametrize("r,E", [(2, 1), (19, 64)])
def test_no_inflation_and_no_observation_is_the_exact_identity(hip_lib, r, E):
    Y, _, R = seeded(r, E, 5)
    yo = np.full(E, np.nan)
    W, stats = ref.weights(Y, yo, R, 1.0)
    got_W, got_stats = weights_host(hip_lib, Y, yo, R, 1.0)
    assert np.array_equal(bits(W), bits(np.eye(r))) and np.array_equal(bits(got_W), bits(np.eye(r)))
    assert np.array_equal(bits(got_stats), bits(stats)) and not stats[:, 2:].any() and (stats[:, 1] > 0).all()
    # (the prior statistics are those of Y itself)
    assert np.allclose(stats[:, 0], Y.mean(axis=1), rtol=1e-14) and np.allclose(stats[:, 1], Y.var(axis=1, ddof=1), rtol=1e-12)


def test_weights_host_checks_its_arguments(hip_lib):
    one = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    assert hip_lib.spd_assim_weights_host(one, 1, 1, one, one, 1.0, one, one) == -1
    assert b"spd_assim_weights_host: r must be 2 ... 64, got 1" in hip_lib.spd_last_error()
    assert hip_lib.spd_assim_weights_host(one, 1, 65, one, one, 1.0, one, one) == -1
    assert hip_lib.spd_assim_weights_host(one, 0, 2, one, one, 1.0, one, one) == -1
    assert b"spd_assim_weights_host: n_entries must be 1 ... 64, got 0" in hip_lib.spd_last_error()
    assert hip_lib.spd_assim_weights_host(None, 1, 2, one, one, 1.0, one, one) == -1
    assert b"spd_assim_weights_host: null argument" in hip_lib.spd_last_error()


# ---- the arbiter on its own -----------------------------------------------------------------------------------------------------
def test_arbiter_is_the_batch_kalman_update_in_observation_space():
    """Independent of the library.  r = 20 members, E = 5 observed quantities, H = I, R diagonal and equal to the prior variances,
    rho = 1.  Textbook: with ybar and P the sample mean and covariance of Y (divisor r - 1) and C = P + R, the posterior mean is
    ybar + P C^-1 (yo - ybar) and the posterior covariance P - P C^-1 P, both through np.linalg.solve.  The serial square-root
    filter with a diagonal R is that update in exact arithmetic, so mean and covariance of Y W are compared with it.  Bound:
    64 E r kappa(C) 2^-53 -- the form DESIGN 4k uses for its QR comparison: E r operations feed an entry, the solve amplifies by
    kappa(C) -- relative to the largest posterior standard deviation sigma (the mean) and to sigma^2 (the covariance).  Column sums
    of W are 1 within the same bound.  The bound has no term for the size of the rows' means against their spread (deviations
    y_j - ybar of a row with |ybar| = 1000 sigma lose three digits, in the filter and in the textbook alike), so the rows' means
    are of their spreads' size.  Observed: kappa(C) = 7.03, bound 5.0e-12; mean 4.6e-17, covariance 3.8e-16, column sums 4.4e-16."""
    r, E = 20, 5
    rng = np.random.default_rng(42)
    scale = np.array([1.0, 1.5, 2.0, 2.5, 3.0])[:, None]
    Y = np.array([0.5, -1.0, 2.0, 0.0, -3.0])[:, None] + scale * rng.standard_normal((E, r))  # rows drawn independently
    P = np.cov(Y, ddof=1)
    R = np.diag(P).copy()
    yo = Y.mean(axis=1) + np.sqrt(R) * rng.standard_normal(E)
    W, stats = ref.weights(Y, yo, R, 1.0)
    assert stats[:, 3].all()
    Ya = Y @ W
    Cm = P + np.diag(R)
    kappa = np.linalg.cond(Cm)
    mean_want = Y.mean(axis=1) + P @ np.linalg.solve(Cm, yo - Y.mean(axis=1))
    cov_want = P - P @ np.linalg.solve(Cm, P)
    sigma = float(np.sqrt(np.diag(cov_want)).max())
    bound = 64 * E * r * kappa * 2.0 ** -53
    err_mean = float(np.abs(Ya.mean(axis=1) - mean_want).max()) / sigma
    err_cov = float(np.abs(np.cov(Ya, ddof=1) - cov_want).max()) / sigma ** 2
    err_sum = float(np.abs(W.sum(axis=0) - 1.0).max())
    print("kappa(C) = %.3g, bound %.2e: mean %.2e, covariance %.2e, column sums %.2e" % (kappa, bound, err_mean, err_cov, err_sum))
    assert kappa < 100.0  # (well conditioned: the rows are independent and R is of P's size)
    assert err_mean <= bound and err_cov <= bound and err_sum <= bound, (err_mean, err_cov, err_sum, bound)
    # the first entry's prior statistics are Y's own; a later one's are those of the updated ensemble
    assert abs(stats[0, 0] - Y[0].mean()) <= 1e-13 * abs(Y[0].mean()) and abs(stats[0, 1] / P[0, 0] - 1.0) < 1e-13
    assert np.all(np.diag(cov_want) < np.diag(P))


def test_arbiter_transform_is_the_matrix_product_inside_the_truncation():
    rng = np.random.default_rng(3)
    shape = {"vor": (31, 32, 8, 2), "div": (31, 32, 8, 2), "t": (31, 32, 8, 2), "tr": (31, 32, 8, 2), "ps": (31, 32, 2)}
    states = [{n: rng.standard_normal(s) + 1j * rng.standard_normal(s) for n, s in shape.items()} for _ in range(3)]
    W = rng.standard_normal((3, 3))
    moved = ref.transform(states, W)
    for n in ref.NAMES:
        stack = np.stack([x[n] for x in states], axis=-1)
        for j in range(3):
            want = stack @ W[:, j]
            assert np.allclose(moved[j][n][ref.INSIDE], want[ref.INSIDE], rtol=1e-13, atol=1e-13)
            assert np.array_equal(moved[j][n][~ref.INSIDE], states[j][n][~ref.INSIDE])
    same = ref.transform(states, np.eye(3))
    assert all(np.array_equal(bits(same[j][n].view(np.float64)), bits(states[j][n].view(np.float64))) for j in range(3) for n in ref.NAMES)


# ---- the argument checks without a model ----------------------------------------------------------------------------------------
def check(hip_lib, weights=None, entries=(("t_grid", 7, 0),), mask=(0, 1, 1), every=4, capacity=8, inflation=1.0, in_loop=1):
    w = np.ones((1, 48, 96)) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    n = max(len(entries), 1)
    names = (C.c_char_p * n)(*[e[0].encode() for e in entries])
    levels = (C.c_int * n)(*[e[1] for e in entries])
    patterns = (C.c_int * n)(*[e[2] for e in entries])
    m = None if mask is None else np.asarray(mask, dtype=np.int32)
    rc = hip_lib.spd_assim_check(as_double(w), w.shape[0], names, levels, patterns, len(entries),
                                 None if m is None else m.ctypes.data_as(C.POINTER(C.c_int32)), 0 if m is None else len(m), every, capacity,
                                 inflation, in_loop)
    return rc, hip_lib.spd_last_error()


def test_assim_check(hip_lib):
    assert check(hip_lib)[0] == 0
    assert check(hip_lib, mask=None)[0] == 0
    many = tuple(("t_grid", k % 8, 0) for k in range(64))
    assert check(hip_lib, entries=many, mask=[0] + [1] * 64 + [0])[0] == 0  # r = 64, E = 64
    bad = np.ones((2, 48, 96))
    bad[1, 5, 7] = np.inf
    for kwargs, message in ((dict(mask=(0, 1, 0)), b"1 members are masked in: an analysis takes 2 ... 64"),
                            (dict(mask=[1] * 65), b"65 members are masked in: an analysis takes 2 ... 64"),
                            (dict(mask=(0, 2, 1)), b"the mask of member 1 (2) is not 0 or 1"),
                            (dict(entries=()), b"n_entries must be 1 ... 64, got 0"),
                            (dict(entries=many + (("t_grid", 0, 0),)), b"n_entries must be 1 ... 64, got 65"),
                            (dict(entries=(("t_grid", 7, 0), ("precnv", 0, 0))), b"'precnv' (entry 1) cannot be assimilated"),
                            (dict(entries=(("precls", 0, 0),)), b"'precls' (entry 0) cannot be assimilated"),
                            (dict(entries=(("vorticity", 0, 0),)), b"unknown variable 'vorticity'"),
                            (dict(entries=(("t_grid", 8, 0),)), b"level 8 of entry 0 ('t_grid') is out of range (0 ... 7)"),
                            (dict(entries=(("t_grid", 0, 1),)), b"pattern 1 of entry 0 ('t_grid') is out of range (0 ... 0)"),
                            (dict(weights=bad), b"weight of pattern 1 at point 487 (row 5, column 7) is not finite"),
                            (dict(weights=np.ones((65, 48, 96))), b"n_patterns must be 1 ... 64, got 65"),
                            (dict(inflation=0.99), b"inflation must be a finite number >= 1"),
                            (dict(inflation=np.nan), b"inflation must be a finite number >= 1"),
                            (dict(inflation=np.inf), b"inflation must be a finite number >= 1"),
                            (dict(every=0), b"every must be at least 1"),
                            (dict(capacity=0), b"capacity must be at least 1"),
                            (dict(in_loop=2), b"in_loop must be 0 or 1")):
        rc, text = check(hip_lib, **kwargs)
        assert rc == -1 and text.startswith(b"spd_model_assim_configure: ") and message in text, (kwargs.keys(), text)
    # the documented order: every before the inflation before the entries before the mask
    assert b"every must" in check(hip_lib, every=0, inflation=0.5, entries=(), mask=(1,))[1]
    assert b"inflation must" in check(hip_lib, inflation=0.5, entries=(), mask=(1,))[1]
    assert b"n_entries must" in check(hip_lib, entries=(), mask=(1,))[1]


def upload(hip_lib, steps, yo, var, entries=None):
    steps = np.asarray(steps, dtype=np.int32)
    yo, var = np.ascontiguousarray(yo, dtype=np.float64), np.ascontiguousarray(var, dtype=np.float64)
    rc = hip_lib.spd_model_assim_set_observations(None, steps.ctypes.data_as(C.POINTER(C.c_int32)), len(steps), as_double(yo), as_double(var),
                                                  yo.shape[1] if entries is None else entries)
    return rc, hip_lib.spd_last_error()


def test_observation_upload_checks_the_table_before_the_model(hip_lib):
    yo, var = np.zeros((3, 2)), np.ones((3, 2))
    rc, text = upload(hip_lib, [32, 40, 48], yo, var)
    assert rc == -1 and b"spd_model_assim_set_observations: null model" in text  # (the table passed)
    missing = yo.copy()
    missing[1, 1] = np.nan
    assert b"null model" in upload(hip_lib, [32, 40, 48], missing, var)[1]  # (NaN means missing)
    for bad in (0.0, -1.0, np.inf, np.nan):
        v = var.copy()
        v[2, 1] = bad
        rc, text = upload(hip_lib, [32, 40, 48], yo, v)
        assert rc == -1 and b"the error variance of row 2, entry 1 is not a finite number > 0" in text, text
    for bad in (np.inf, -np.inf):
        y = yo.copy()
        y[0, 1] = bad
        rc, text = upload(hip_lib, [32, 40, 48], y, var)
        assert rc == -1 and b"the observation of row 0, entry 1 is infinite" in text, text
    rc, text = upload(hip_lib, [32, 48, 40], yo, var)
    assert rc == -1 and b"the step stamps must be strictly ascending (row 2: 40 after 48)" in text
    assert b"strictly ascending (row 1: 32 after 32)" in upload(hip_lib, [32, 32, 40], yo, var)[1]
    assert b"n_entries must be 1 ... 64, got 65" in upload(hip_lib, [32, 40, 48], yo, var, entries=65)[1]
    # the stamps come before the values
    v = var.copy()
    v[0, 0] = 0.0
    assert b"strictly ascending" in upload(hip_lib, [32, 48, 40], yo, v)[1]


# ---- the symbols, the null model, the example ----------------------------------------------------------------------------------
def test_assim_symbols_declared_exported_and_bound(hip_lib):
    import inspect

    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in ASSIM_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for method in ("assim_configure", "assim_observations", "assim_apply", "assim_compute", "assim_transform", "assim", "assim_times",
                   "assim_weights", "assim_info", "assim_reset", "assim_off"):
        assert hasattr(EnsembleModel, method), method
    configure = inspect.signature(EnsembleModel.assim_configure).parameters
    assert list(configure)[1:] == ["weights", "entries", "members", "every", "capacity", "inflation", "in_loop"]
    assert (configure["capacity"].default, configure["inflation"].default, configure["in_loop"].default) == (64, 1.0, True)


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    n = C.c_int()
    one = np.ones((1, 48, 96))
    names, zero = (C.c_char_p * 1)(b"t_grid"), (C.c_int * 1)(0)
    mask = (C.c_int32 * 2)(1, 1)
    assert hip_lib.spd_model_assim_configure(None, as_double(one), 1, names, zero, zero, 1, mask, 4, 8, 1.0, 1) == -1
    assert b"spd_model_assim_configure: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_assim_configure(None, as_double(one), 1, names, zero, zero, 1, None, 4, 8, 1.0, 1) == -1
    assert b"spd_model_assim_configure: null member mask" in hip_lib.spd_last_error()
    for call, args in (("apply", (None,)), ("compute", (None, 0, None)), ("read", (0, 0, None, 0, None)),
                       ("weights", (None, 0, None, 0, None)), ("rows", (None, 0)), ("reset", ()), ("off", ()),
                       ("info", (C.byref(n), None, None, None, None, None, None, None))):
        symbol = "spd_model_assim_" + call
        assert getattr(hip_lib, symbol)(None, *args) == -1, symbol
        assert (symbol + ": null model").encode() in hip_lib.spd_last_error(), symbol
    w = np.eye(2)
    members = (C.c_int32 * 2)(0, 1)
    assert hip_lib.spd_model_assim_transform(None, members, 2, as_double(w), None) == -1
    assert b"spd_model_assim_transform: null model" in hip_lib.spd_last_error()
    # ... behind the checks of its arguments
    assert hip_lib.spd_model_assim_transform(None, members, 65, as_double(w), None) == -1
    assert b"spd_model_assim_transform: r must be 1 ... 64, got 65" in hip_lib.spd_last_error()
    w[1, 0] = np.nan
    assert hip_lib.spd_model_assim_transform(None, members, 2, as_double(w), None) == -1
    assert b"spd_model_assim_transform: W[1][0] is not finite" in hip_lib.spd_last_error()
    twice = (C.c_int32 * 2)(3, 3)
    assert hip_lib.spd_model_assim_transform(None, twice, 2, as_double(np.eye(2)), None) == -1
    assert b"spd_model_assim_transform: member 3 is named twice" in hip_lib.spd_last_error()


def test_osse_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("osse_ensrf", os.path.join(ROOT, "examples", "osse_ensrf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.steps, args.every, args.inflation, args.seed) == (20, 360, 9, 1.02, 0)
    args = mod.parse(["--members", "63", "--steps", "720", "--every", "36", "--inflation", "1.1", "--seed", "7"])
    assert (args.members, args.steps, args.every, args.inflation, args.seed) == (63, 720, 36, 1.1, 7)
    assert mod.mask_of(3).tolist() == [0, 1, 1, 1]
    names = [e[0] for e in mod.ENTRIES]
    assert len(mod.ENTRIES) == len(mod.SIGMA) >= 4 and "precnv" not in names and all(s > 0 for s in mod.SIGMA)
    for bad in (["--members", "1"], ["--members", "64"], ["--every", "0"], ["--inflation", "0.9"], ["--steps", "0"]):
        with pytest.raises(SystemExit):
            mod.parse(bad)
