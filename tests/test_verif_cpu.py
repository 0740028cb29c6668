"""CPU tier: the verification tape.  The arbiter (tests/verif_reference.py, written from the definition with
explicit loops) against the host compile of the device's routines (spd_verif_host), bit for bit; the arbiter on its own against
the textbook forms of mean, variance and CRPS; exact cases; the argument checks without a model (spd_verif_check); the entry
points are declared, exported and bound; calls on a null model; the example parses its arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import verif_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIF_SYMBOLS = ("spd_verif_check", "spd_model_verif_configure", "spd_model_verif_off", "spd_model_verif_reset", "spd_model_verif_apply",
                 "spd_model_verif_compute", "spd_model_verif_read", "spd_model_verif_hist", "spd_model_verif_rows", "spd_model_verif_info",
                 "spd_verif_host")
NG = 4608
EPS = 2.0 ** -52  # (as the ensemble tape's test)
SIZES = (2, 3, 19, 64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def as_double(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def host(hip_lib, x, y, w):
    x, y, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, w))
    out, hist = np.full(4, -7.0), np.full(ref.COUNTS, -7, dtype=np.int32)
    rc = hip_lib.spd_verif_host(as_double(x), x.shape[0], as_double(y), as_double(w), as_double(out), hist.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, hip_lib.spd_last_error()
    return out, hist


def seeded(r, seed):
    """planes of both signs with a scale and an offset of their own at every point, the truth within the ensemble's reach (every
    rank occurs), a weight map of both signs with a block of zeros"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3.0, 3.0, NG)
    centre = scale * rng.standard_normal(NG) * rng.choice([0.0, 1.0, 30.0], NG)
    x = centre + scale * rng.standard_normal((r, NG))
    y = centre + scale * 1.5 * rng.standard_normal(NG)
    w = rng.standard_normal(NG)
    w[rng.choice(NG, 700, replace=False)] = 0.0
    return x, y, w


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    r = request.param
    x, y, w = seeded(r, 400 + r)
    return r, x, y, w, ref.points(x, y), ref.score(x, y, w)


# ---- the library's host compile against the arbiter, bit for bit ---------------------------------------------------------------
def test_host_routine_is_the_arbiter_bit_for_bit(hip_lib, case):
    r, x, y, w, _, (want, want_hist) = case
    got, got_hist = host(hip_lib, x, y, w)
    assert np.isfinite(want).all() and want.all()
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert np.array_equal(got_hist, want_hist), (got_hist, want_hist)
    assert int(want_hist.sum()) == int(np.count_nonzero(w)) == NG - 700  # every point with w != 0 is counted once
    assert want_hist[r + 1] == 0 and not want_hist[r + 2:].any()          # (a continuous case has no tie)
    assert (want_hist[:r + 1] > 0).all()                                  # every rank occurs: the histogram is not a constant


def test_arbiter_vectorised_is_the_loop_over_python_floats(case):
    r, x, y, _, scored, _ = case
    for p in (0, 1, 255, 256, 2047, NG - 1):
        e, se, v, crps, rank, tie = ref.point_loop(x[:, p], y[p])
        got = [scored[k][p] for k in ("e", "se", "v", "crps")]
        assert np.array_equal(bits(got), bits([e, se, v, crps])), p
        assert (int(scored["rank"][p]), bool(scored["tie"][p])) == (rank, tie)


def test_plain_numpy_sums_give_other_bits(case):
    """np.sum adds pairwise in blocks of its own choosing: not the stated order."""
    _, x, y, w, scored, (want, _) = case
    plain = [float(np.sum(w * scored[k])) for k in ("e", "se", "v", "crps")]
    assert not np.array_equal(bits(plain), bits(want))
    assert np.allclose(plain, want, rtol=1e-9)


# ---- the arbiter on its own against the textbook ------------------------------------------------------------------------------
def test_arbiter_mean_and_variance_against_numpy(case):
    """The ensemble tape's bounds: the mean within 4 r eps max|x|, the variance within 16 r eps (v + |mean| sqrt(v))."""
    r, x, y, _, scored, _ = case
    err_mean = np.abs(scored["mean"] - x.mean(axis=0))
    assert (err_mean <= 4 * r * EPS * np.abs(x).max(axis=0)).all(), float(err_mean.max())
    assert np.array_equal(bits(scored["e"]), bits(scored["mean"] - y))
    v = x.var(axis=0, ddof=1)
    err_var = np.abs(scored["v"] - v)
    assert (err_var <= 16 * r * EPS * (v + np.abs(x.mean(axis=0)) * np.sqrt(v))).all(), float(err_var.max())
    assert np.array_equal(bits(scored["se"]), bits(scored["e"] * scored["e"]))


def test_arbiter_crps_against_the_sorted_sample_form(case):
    """CRPS = (1 / r) sum |x_j - y| - (1 / r^2) sum_i (2 i - r - 1) x_(i), i = 1 ... r over the sorted sample -- the same quantity
    without the pair loop.  Bound 2 r^2 eps max |a - b| over the values at the point (the truth among them): the first-order bound
    of r^2 / 2 rounded terms of that size."""
    r, x, y, _, scored, _ = case
    srt = np.sort(x, axis=0)
    i = np.arange(1, r + 1)[:, None]
    textbook = np.abs(x - y).mean(axis=0) - ((2 * i - r - 1) * srt).sum(axis=0) / r ** 2
    both = np.concatenate([x, y[None]])
    reach = both.max(axis=0) - both.min(axis=0)
    err = np.abs(scored["crps"] - textbook)
    print("r = %d: largest error %.2e of the bound" % (r, float((err / (2 * r * r * EPS * reach)).max())))
    assert (err <= 2 * r * r * EPS * reach).all()
    assert (scored["crps"] > 0).all()
    ranks = (x < y).sum(axis=0)
    assert np.array_equal(scored["rank"], ranks) and not scored["tie"].any()


# ---- exact cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [2, 4])
def test_members_equal_to_the_truth_score_exactly_zero(hip_lib, r):
    """r = 2 and r = 4: y + y is exact, fl(3 y) + y rounds to 4 y (the error of fl(3 y) is at most half an ulp of 4 y, and where it
    is exactly half, 4 y is the even neighbour), and the division by a power of two is exact, so mean == y bitwise.  For other r
    the rounded mean of r copies of y need not be y (r = 3: fl(fl(3 y) / 3) != y for some y), and the definition then gives a bias
    of an ulp, as it should."""
    _, y, w = seeded(r, 7)
    x = np.repeat(y[None], r, axis=0)
    for out, hist in (ref.score(x, y, w), host(hip_lib, x, y, w)):
        assert np.array_equal(bits(out), bits(np.zeros(4)))
        assert hist[r + 1] == np.count_nonzero(w) and not hist[:r + 1].any() and not hist[r + 2:].any()


def test_four_identical_members_off_the_truth(hip_lib):
    """r = 4: the sum of four equal values and its division by four are exact, so the mean is x, the variance 0 and the CRPS
    bitwise |x - y| at every point; under a map with one unit weight the entry is that point's value."""
    _, y, _ = seeded(4, 11)
    rng = np.random.default_rng(12)
    one = rng.standard_normal(NG) * 10.0 ** rng.uniform(-3, 3, NG)
    x = np.repeat(one[None], 4, axis=0)
    scored = ref.points(x, y)
    assert np.array_equal(bits(scored["v"]), bits(np.zeros(NG)))
    assert np.array_equal(bits(scored["crps"]), bits(np.abs(one - y)))
    assert np.array_equal(scored["rank"], np.where(one < y, 4, 0)) and not scored["tie"].any()
    for p in (0, 300, NG - 1):
        w = np.zeros(NG)
        w[p] = 1.0
        for out, hist in (ref.score(x, y, w), host(hip_lib, x, y, w)):
            assert out[2] == 0.0 and bits(out[3]) == bits(abs(one[p] - y[p])) and bits(out[0]) == bits(one[p] - y[p])
            assert hist.sum() == 1 and hist[4 if one[p] < y[p] else 0] == 1


def test_ties_are_counted_apart_and_only_under_a_weight(hip_lib):
    r = 5
    x, y, w = seeded(r, 21)
    tied = np.arange(0, NG, 7)
    x[2, tied] = y[tied]
    out, hist = ref.score(x, y, w)
    got, got_hist = host(hip_lib, x, y, w)
    assert np.array_equal(bits(got), bits(out)) and np.array_equal(got_hist, hist)
    assert hist[r + 1] == np.count_nonzero(w[tied]) > 0
    assert hist.sum() == np.count_nonzero(w)


def test_host_routine_checks_its_arguments(hip_lib):
    one = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    hist = (C.c_int32 * 66)()
    assert hip_lib.spd_verif_host(one, 1, one, one, one, hist) == -1
    assert b"spd_verif_host: r must be 2 ... 64, got 1" in hip_lib.spd_last_error()
    assert hip_lib.spd_verif_host(one, 65, one, one, one, hist) == -1
    assert hip_lib.spd_verif_host(None, 2, one, one, one, hist) == -1
    assert b"spd_verif_host: null argument" in hip_lib.spd_last_error()
    assert hip_lib.spd_verif_host(one, 2, one, one, one, None) == -1


# ---- the argument checks without a model ----------------------------------------------------------------------------------------
def check(hip_lib, weights=None, entries=(("t_grid", 7, 0),), mask=(0, 1, 1), truth=0, every=4, capacity=8, in_loop=1):
    w = np.ones((1, 48, 96)) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    n = max(len(entries), 1)
    names = (C.c_char_p * n)(*[e[0].encode() for e in entries])
    levels = (C.c_int * n)(*[e[1] for e in entries])
    patterns = (C.c_int * n)(*[e[2] for e in entries])
    m = None if mask is None else np.asarray(mask, dtype=np.int32)
    rc = hip_lib.spd_verif_check(as_double(w), w.shape[0], names, levels, patterns, len(entries),
                                 None if m is None else m.ctypes.data_as(C.POINTER(C.c_int32)), 0 if m is None else len(m), truth, every,
                                 capacity, in_loop)
    return rc, hip_lib.spd_last_error()


def test_verif_check(hip_lib):
    assert check(hip_lib)[0] == 0
    assert check(hip_lib, mask=None)[0] == 0
    many = tuple(("t_grid", k % 8, 0) for k in range(256))
    assert check(hip_lib, entries=many, mask=[0] + [1] * 64 + [0], truth=65)[0] == 0  # r = 64, E = 256
    assert check(hip_lib, entries=(("precnv", 0, 0), ("z_plev", 3, 0), ("tcwv", 0, 0)))[0] == 0  # (the projection tape's names)
    bad = np.ones((2, 48, 96))
    bad[1, 5, 7] = np.inf
    for kwargs, message in ((dict(mask=(0, 1, 0)), b"1 members are masked in: the scores take 2 ... 64"),
                            (dict(mask=[0] + [1] * 65), b"65 members are masked in: the scores take 2 ... 64"),
                            (dict(mask=(0, 2, 1)), b"the mask of member 1 (2) is not 0 or 1"),
                            (dict(truth=1), b"the truth member 1 is masked in"),
                            (dict(truth=3), b"the truth member 3 is out of range (0 ... 2)"),
                            (dict(truth=-1), b"the truth member -1 is out of range (0 ... 2)"),
                            (dict(entries=()), b"n_entries must be 1 ... 256, got 0"),
                            (dict(entries=many + (("t_grid", 0, 0),)), b"n_entries must be 1 ... 256, got 257"),
                            (dict(entries=(("vorticity", 0, 0),)), b"unknown variable 'vorticity'"),
                            (dict(entries=(("t_grid", 8, 0),)), b"level 8 of entry 0 ('t_grid') is out of range (0 ... 7)"),
                            (dict(entries=(("t_grid", 0, 1),)), b"pattern 1 of entry 0 ('t_grid') is out of range (0 ... 0)"),
                            (dict(weights=bad), b"weight of pattern 1 at point 487 (row 5, column 7) is not finite"),
                            (dict(weights=np.ones((65, 48, 96))), b"n_patterns must be 1 ... 64, got 65"),
                            (dict(every=0), b"every must be at least 1"),
                            (dict(capacity=0), b"capacity must be at least 1"),
                            (dict(in_loop=2), b"in_loop must be 0 or 1")):
        rc, text = check(hip_lib, **kwargs)
        assert rc == -1 and text.startswith(b"spd_model_verif_configure: ") and message in text, (kwargs.keys(), text)
    # the documented order: every before the entries before the mask before the truth
    assert b"every must" in check(hip_lib, every=0, entries=(), mask=(1,), truth=5)[1]
    assert b"n_entries must" in check(hip_lib, entries=(), mask=(1,), truth=5)[1]
    assert b"members are masked in" in check(hip_lib, mask=(1,), truth=5)[1]
    assert b"is out of range" in check(hip_lib, mask=(1, 1), truth=5)[1]


# ---- the symbols, the null model, the example ----------------------------------------------------------------------------------
def test_verif_symbols_declared_exported_and_bound(hip_lib):
    import inspect

    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in VERIF_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for method in ("verif_configure", "verif_off", "verif_reset", "verif_apply", "verif_compute", "verif_info", "verif", "verif_hist",
                   "verif_steps", "verif_times", "verif_entries"):
        assert hasattr(EnsembleModel, method), method
    configure = inspect.signature(EnsembleModel.verif_configure).parameters
    assert list(configure)[1:] == ["weights", "entries", "members", "truth", "every", "capacity", "in_loop"]
    assert (configure["capacity"].default, configure["in_loop"].default) == (64, True)


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    n = C.c_int()
    one = np.ones((1, 48, 96))
    names, zero = (C.c_char_p * 1)(b"t_grid"), (C.c_int * 1)(0)
    mask = (C.c_int32 * 3)(0, 1, 1)
    assert hip_lib.spd_model_verif_configure(None, as_double(one), 1, names, zero, zero, 1, mask, 0, 4, 8, 1) == -1
    assert b"spd_model_verif_configure: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_verif_configure(None, as_double(one), 1, names, zero, zero, 1, None, 0, 4, 8, 1) == -1
    assert b"spd_model_verif_configure: null member mask" in hip_lib.spd_last_error()
    # ... behind the checks of the arguments
    assert hip_lib.spd_model_verif_configure(None, as_double(one), 1, names, zero, zero, 1, mask, 0, 0, 8, 1) == -1
    assert b"every must be at least 1" in hip_lib.spd_last_error()
    for call, args in (("apply", (None,)), ("compute", (None, 0, None, 0, None)), ("read", (0, 0, None, 0, None)),
                       ("hist", (0, 0, None, 0, None)), ("rows", (None, 0)), ("reset", ()), ("off", ()),
                       ("info", (C.byref(n), None, None, None, None, None, None, None))):
        symbol = "spd_model_verif_" + call
        assert getattr(hip_lib, symbol)(None, *args) == -1, symbol
        assert (symbol + ": null model").encode() in hip_lib.spd_last_error(), symbol


def test_scores_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("osse_scores", os.path.join(ROOT, "examples", "osse_scores.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.steps, args.every, args.inflation, args.seed) == (20, 360, 9, 1.02, 0)
    args = mod.parse(["--members", "63", "--steps", "720", "--every", "36", "--inflation", "1.1", "--seed", "7"])
    assert (args.members, args.steps, args.every, args.inflation, args.seed) == (63, 720, 36, 1.1, 7)
    assert mod.mask_of(3).tolist() == [0, 1, 1, 1]
    assert [s[0] for s in mod.SCORED] == ["T850", "Z500"] and [g[0] for g in mod.REGIONS] == ["NH", "tropics", "SH"]
    assert len(mod.score_entries()) == len(mod.SCORED) * len(mod.REGIONS)
    for bad in (["--members", "1"], ["--members", "64"], ["--every", "0"], ["--inflation", "0.9"], ["--steps", "0"]):
        with pytest.raises(SystemExit):
            mod.parse(bad)
