"""CPU tier: the quantile tape.  The host compile of the device's routines (spd_qtape_host) against the arbiter
(tests/qtape_reference.py: numpy's stable sort and one elementwise operation per line of the definition), bit for bit; the
arbiter on its own against np.min / np.max / np.mean / np.quantile; properties of both; the argument checks without a model
(spd_qtape_check); the entry points are declared, exported and bound; calls on a null model; the example parses its arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import qtape_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QTAPE_SYMBOLS = ("spd_qtape_check", "spd_model_qtape_configure", "spd_model_qtape_off", "spd_model_qtape_reset", "spd_model_qtape_apply",
                 "spd_model_qtape_compute", "spd_model_qtape_read", "spd_model_qtape_rows", "spd_model_qtape_info", "spd_qtape_host")
NG = 4608
EPS = 2.0 ** -52
SIZES = (2, 3, 19, 64)
QS = (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.9, 1.0)
ELEVEN = tuple(k / 10.0 for k in range(11))
THR = (0.375, -12.5)  # thresholds that members equal at planted points


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def as_double(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def host(hip_lib, x, entries):
    """entries: (op, param) -> float64 [E][4608] from the library's host compile"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(entries)
    ops = (C.c_int * n)(*[ref.OPS[op] for op, _ in entries])
    params = (C.c_double * n)(*[float(p) for _, p in entries])
    out = np.full((n, NG), -7.0)
    rc = hip_lib.spd_qtape_host(as_double(x), x.shape[0], ops, params, n, as_double(out))
    assert rc == 0, hip_lib.spd_last_error()
    return out


def arbiter(x, entries):
    return np.stack([ref.value(x, op, param) for op, param in entries])


def seeded(r, seed, plant=True):
    """planes of both signs with a scale of their own at every point (1e-3 ... 1e3); planted: a duplicate between two members at
    every seventh point, a (-0.0, +0.0) pair in members (0, 1) -- in the other order at every 22nd point -- with the other members
    all positive or all negative at every eleventh, and a member equal to each threshold at every 13th / 17th point"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3.0, 3.0, NG)
    x = scale * rng.standard_normal((r, NG))
    if not plant:
        return x
    p = duplicate_points()
    x[(p // 7) % r, p] = x[(p // 7 + 1) % r, p]
    for k, thr in enumerate(THR):
        p = threshold_points(k)
        x[(p // 13 + k) % r, p] = thr  # (a point planted for both thresholds holds them in two members)
    p = np.arange(0, NG, 11)
    side = np.where((p // 11) % 3 == 0, -1.0, 1.0)
    x[:, p] = side * (np.abs(x[:, p]) + 1e-3)
    x[0, p], x[1, p] = -0.0, 0.0
    swapped = p[p % 22 == 0]
    x[0, swapped], x[1, swapped] = 0.0, -0.0
    return x


def duplicate_points():
    p = np.arange(0, NG, 7)
    return p[p % 11 != 0]


def threshold_points(k):
    p = np.arange(3 + k, NG, 13 + 4 * k)
    return p[(p % 11 != 0) & (p % 7 != 0)]


def all_entries():
    return ([("min", 0.0), ("max", 0.0)] + [("quantile", q) for q in QS] +
            [("prob_above", THR[0]), ("prob_below", THR[0]), ("prob_above", THR[1]), ("prob_below", THR[1]), ("prob_above", 0.0),
             ("prob_below", 0.0)])


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    r = request.param
    return r, seeded(r, 900 + r)


# ---- the library's host compile against the arbiter, bit for bit ---------------------------------------------------------------
def test_host_routine_is_the_arbiter_bit_for_bit(hip_lib, case):
    r, x = case
    entries = all_entries()
    got, want = host(hip_lib, x, entries), arbiter(x, entries)
    assert np.isfinite(want).all()
    for k, entry in enumerate(entries):
        assert np.array_equal(bits(got[k]), bits(want[k])), (entry, int((bits(got[k]) != bits(want[k])).sum()))
    # the planted cases took part: both signs of zero among the minima and the maxima, in the order of the member index
    zero = np.arange(0, NG, 11)
    lowest, highest = want[0][zero], want[1][zero]
    first, second = x[0, zero], x[1, zero]
    low = (x[2:, zero] > 0).all(axis=0) if r > 2 else np.ones(len(zero), dtype=bool)
    high = (x[2:, zero] < 0).all(axis=0) if r > 2 else np.ones(len(zero), dtype=bool)
    assert np.array_equal(bits(lowest[low]), bits(first[low])) and np.array_equal(bits(highest[high]), bits(second[high]))
    assert {0, 1} <= set(np.signbit(lowest[low]).tolist()) and {0, 1} <= set(np.signbit(highest[high]).tolist())
    # strictness: a member that equals the threshold is counted neither above nor below
    for k, thr in enumerate(THR):
        at = threshold_points(k)
        above, below, equal = want[9 + 2 * k][at], want[10 + 2 * k][at], (x[:, at] == thr).sum(axis=0)
        assert len(at) > 100 and (equal >= 1).all()
        assert np.array_equal(np.rint(above * r) + np.rint(below * r) + equal, np.full(len(at), r))
        assert np.array_equal(above, (x[:, at] > thr).sum(axis=0) / r) and np.array_equal(below, (x[:, at] < thr).sum(axis=0) / r)
    dup = duplicate_points()
    assert (np.array([len(set(x[:, q].tolist())) for q in dup]) < r).all()  # (the duplicates took part)


# ---- the arbiter on its own against numpy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [2, 3, 5, 19, 64])
def test_arbiter_against_numpy(r):
    """min / max are np.min / np.max and the probabilities np.mean(x > thr) bitwise; the quantile lies within 8 eps max_j |x_j| of
    np.quantile: three roundings of terms <= 2 max|x| on each side, 6 eps, rounded up."""
    x = seeded(r, 40 + r, plant=False)  # (no signed zeros: np.min does not say which zero it returns)
    assert np.array_equal(bits(ref.value(x, "min")), bits(np.min(x, axis=0)))
    assert np.array_equal(bits(ref.value(x, "max")), bits(np.max(x, axis=0)))
    for thr in (0.0, 0.01, -3.0):
        assert np.array_equal(bits(ref.value(x, "prob_above", thr)), bits(np.mean(x > thr, axis=0)))
        assert np.array_equal(bits(ref.value(x, "prob_below", thr)), bits(np.mean(x < thr, axis=0)))
    reach = np.abs(x).max(axis=0)
    worst = 0.0
    for q in (0.0, 0.05, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.9, 1.0):
        err = np.abs(ref.value(x, "quantile", q) - np.quantile(x, q, axis=0))
        worst = max(worst, float((err / (EPS * reach)).max()))
        assert (err <= 8 * EPS * reach).all(), (q, float((err / (EPS * reach)).max()))
    print("r = %d: the quantile differs from np.quantile by at most %.2f eps max|x|" % (r, worst))


# ---- properties of the arbiter and of the host routine --------------------------------------------------------------------------
def test_quantiles_do_not_decrease_with_q(hip_lib, case):
    r, x = case
    entries = [("quantile", q) for q in ELEVEN]
    for planes in (arbiter(x, entries), host(hip_lib, x, entries)):
        assert (np.diff(planes, axis=0) >= 0).all()
        lo, hi = np.min(x, axis=0), np.max(x, axis=0)
        assert (planes >= lo).all() and (planes <= hi).all()
        assert np.array_equal(planes[0], lo) and np.array_equal(planes[-1], hi)


@pytest.mark.parametrize("r", [3, 19, 63])
def test_the_median_of_an_odd_ensemble_is_its_middle_value(hip_lib, r):
    x = seeded(r, 70 + r)
    middle = np.sort(x, axis=0, kind="stable")[(r - 1) // 2]
    for planes in (arbiter(x, [("quantile", 0.5)]), host(hip_lib, x, [("quantile", 0.5)])):
        assert np.array_equal(bits(planes[0]), bits(middle))


@pytest.mark.parametrize("r", SIZES)
def test_identical_members_give_their_value_and_probabilities_of_zero_or_one(hip_lib, r):
    one = seeded(2, 5, plant=False)[0]
    x = np.repeat(one[None], r, axis=0)
    entries = [("min", 0.0), ("max", 0.0)] + [("quantile", q) for q in ELEVEN + (1.0 / 3.0,)]
    counts = [("prob_above", 0.0), ("prob_below", 0.0), ("prob_above", float(one[17])), ("prob_below", float(one[17]))]
    for f in (arbiter, lambda x, e: host(hip_lib, x, e)):
        planes = f(x, entries)
        assert all(np.array_equal(bits(plane), bits(one)) for plane in planes)
        shares = f(x, counts)
        assert np.isin(shares, (0.0, 1.0)).all()
        assert np.array_equal(shares[0], (one > 0).astype(np.float64)) and np.array_equal(shares[0] + shares[1], np.ones(NG))
        assert shares[2][17] == 0.0 and shares[3][17] == 0.0  # (strict: the value itself is neither above nor below)


def test_host_routine_checks_its_arguments(hip_lib):
    x = (C.c_double * (2 * NG))()
    out = (C.c_double * NG)()
    ops, params = (C.c_int * 1)(2), (C.c_double * 1)(0.5)
    assert hip_lib.spd_qtape_host(x, 2, ops, params, 1, out) == 0
    assert hip_lib.spd_qtape_host(x, 1, ops, params, 1, out) == -1
    assert b"spd_qtape_host: r must be 2 ... 64, got 1" in hip_lib.spd_last_error()
    assert hip_lib.spd_qtape_host(x, 65, ops, params, 1, out) == -1
    assert hip_lib.spd_qtape_host(None, 2, ops, params, 1, out) == -1
    assert b"spd_qtape_host: null argument" in hip_lib.spd_last_error()
    assert hip_lib.spd_qtape_host(x, 2, ops, params, 0, out) == -1
    assert hip_lib.spd_qtape_host(x, 2, (C.c_int * 1)(5), params, 1, out) == -1
    assert b"unknown op 5" in hip_lib.spd_last_error()
    assert hip_lib.spd_qtape_host(x, 2, ops, (C.c_double * 1)(1.5), 1, out) == -1
    assert hip_lib.spd_qtape_host(x, 2, (C.c_int * 1)(3), (C.c_double * 1)(float("inf")), 1, out) == -1


# ---- the argument checks without a model ----------------------------------------------------------------------------------------
def check(hip_lib, entries=(("t_grid", 7, 2, 0.5),), mask=(0, 1, 1), every=4, capacity=8, in_loop=1):
    n = max(len(entries), 1)
    names = (C.c_char_p * n)(*[e[0].encode() for e in entries])
    levels = (C.c_int * n)(*[e[1] for e in entries])
    ops = (C.c_int * n)(*[e[2] for e in entries])
    params = (C.c_double * n)(*[e[3] for e in entries])
    m = None if mask is None else np.asarray(mask, dtype=np.int32)
    rc = hip_lib.spd_qtape_check(names, levels, ops, params, len(entries), None if m is None else m.ctypes.data_as(C.POINTER(C.c_int32)),
                                 0 if m is None else len(m), every, capacity, in_loop)
    return rc, hip_lib.spd_last_error()


def test_qtape_check(hip_lib):
    assert check(hip_lib)[0] == 0
    assert check(hip_lib, mask=None)[0] == 0
    many = tuple(("t_grid", k % 8, k % 2, 0.0) for k in range(64))
    assert check(hip_lib, entries=many, mask=[0] + [1] * 64 + [0])[0] == 0  # r = 64, E = 64
    assert check(hip_lib, entries=(("precnv", 0, 3, 0.0), ("z_plev", 3, 2, 1.0), ("tcwv", 0, 2, 0.0), ("mslp", 0, 4, 101325.0)))[0] == 0
    assert check(hip_lib, entries=(("t_grid", 0, 0, float("nan")), ("t_grid", 0, 1, float("inf"))))[0] == 0  # (min, max read no param)
    for kwargs, message in ((dict(mask=(0, 1, 0)), b"1 members are masked in: the order statistics take 2 ... 64"),
                            (dict(mask=[0] + [1] * 65), b"65 members are masked in: the order statistics take 2 ... 64"),
                            (dict(mask=(0, 2, 1)), b"the mask of member 1 (2) is not 0 or 1"),
                            (dict(entries=()), b"n_entries must be 1 ... 64, got 0"),
                            (dict(entries=many + (("t_grid", 0, 0, 0.0),)), b"n_entries must be 1 ... 64, got 65"),
                            (dict(entries=(("vorticity", 0, 0, 0.0),)), b"unknown variable 'vorticity'"),
                            (dict(entries=(("t_grid", 8, 0, 0.0),)), b"level 8 of entry 0 ('t_grid') is out of range (0 ... 7)"),
                            (dict(entries=(("t_grid", 0, 5, 0.0),)), b"unknown op 5 of entry 0 ('t_grid')"),
                            (dict(entries=(("t_grid", 0, -1, 0.0),)), b"unknown op -1 of entry 0 ('t_grid')"),
                            (dict(entries=(("t_grid", 0, 2, 1.25),)), b"of entry 0 ('t_grid') is not within 0 ... 1"),
                            (dict(entries=(("t_grid", 0, 2, -0.01),)), b"of entry 0 ('t_grid') is not within 0 ... 1"),
                            (dict(entries=(("t_grid", 0, 2, float("nan")),)), b"of entry 0 ('t_grid') is not within 0 ... 1"),
                            (dict(entries=(("t_grid", 0, 2, 0.5), ("mslp", 0, 3, float("inf")))), b"the threshold of entry 1 ('mslp') is not finite"),
                            (dict(entries=(("mslp", 0, 4, float("nan")),)), b"the threshold of entry 0 ('mslp') is not finite"),
                            (dict(every=0), b"every must be at least 1"),
                            (dict(capacity=0), b"capacity must be at least 1"),
                            (dict(in_loop=2), b"in_loop must be 0 or 1")):
        rc, text = check(hip_lib, **kwargs)
        assert rc == -1 and text.startswith(b"spd_model_qtape_configure: ") and message in text, (kwargs.keys(), text)
    # the documented order: every, capacity, in_loop, the entries (name, level, op, param), the mask
    assert b"every must" in check(hip_lib, every=0, capacity=0, entries=(), mask=(1,))[1]
    assert b"capacity must" in check(hip_lib, capacity=0, in_loop=3, entries=(), mask=(1,))[1]
    assert b"in_loop must" in check(hip_lib, in_loop=3, entries=(), mask=(1,))[1]
    assert b"n_entries must" in check(hip_lib, entries=(), mask=(1,))[1]
    assert b"unknown variable" in check(hip_lib, entries=(("nope", 9, 9, 9.0),), mask=(1,))[1]
    assert b"level 9" in check(hip_lib, entries=(("t_grid", 9, 9, 9.0),), mask=(1,))[1]
    assert b"unknown op 9" in check(hip_lib, entries=(("t_grid", 0, 9, 9.0),), mask=(1,))[1]
    assert b"not within 0 ... 1" in check(hip_lib, entries=(("t_grid", 0, 2, 9.0),), mask=(1,))[1]
    assert b"members are masked in" in check(hip_lib, mask=(1,))[1]


# ---- the symbols, the null model, the example ----------------------------------------------------------------------------------
def test_qtape_symbols_declared_exported_and_bound(hip_lib):
    import inspect

    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in QTAPE_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for k, op in enumerate(("SPD_Q_MIN", "SPD_Q_MAX", "SPD_Q_QUANTILE", "SPD_Q_PROB_ABOVE", "SPD_Q_PROB_BELOW")):
        assert "#define %s %d\n" % (op, k) in header and "%s = %d" % (op, k) in fortran and getattr(L, op) == k
    assert EnsembleModel.QTAPE_OPS == ref.OPS
    for method in ("qtape_configure", "qtape_off", "qtape_reset", "qtape_apply", "qtape_compute", "qtape_info", "qtape", "qtape_steps",
                   "qtape_times", "qtape_entries"):
        assert hasattr(EnsembleModel, method), method
    configure = inspect.signature(EnsembleModel.qtape_configure).parameters
    assert list(configure)[1:] == ["entries", "members", "every", "capacity", "in_loop"]
    assert (configure["capacity"].default, configure["in_loop"].default) == (64, True)
    read = inspect.signature(EnsembleModel.qtape).parameters
    assert list(read)[1:] == ["entry", "t0", "nt"] and (read["t0"].default, read["nt"].default) == (0, None)


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    n = C.c_int()
    names, zero, half = (C.c_char_p * 1)(b"t_grid"), (C.c_int * 1)(0), (C.c_double * 1)(0.5)
    mask = (C.c_int32 * 3)(0, 1, 1)
    assert hip_lib.spd_model_qtape_configure(None, names, zero, zero, half, 1, mask, 4, 8, 1) == -1
    assert b"spd_model_qtape_configure: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_qtape_configure(None, names, zero, zero, half, 1, None, 4, 8, 1) == -1
    assert b"spd_model_qtape_configure: null member mask" in hip_lib.spd_last_error()
    # ... behind the checks of the arguments
    assert hip_lib.spd_model_qtape_configure(None, names, zero, zero, half, 1, mask, 0, 8, 1) == -1
    assert b"every must be at least 1" in hip_lib.spd_last_error()
    for call, args in (("apply", (None,)), ("compute", (None, 0, None)), ("read", (0, 0, 0, None, 0, None)), ("rows", (None, 0)),
                       ("reset", ()), ("off", ()), ("info", (C.byref(n), None, None, None, None, None, None))):
        symbol = "spd_model_qtape_" + call
        assert getattr(hip_lib, symbol)(None, *args) == -1, symbol
        assert (symbol + ": null model").encode() in hip_lib.spd_last_error(), symbol


def test_probability_maps_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("probability_maps", os.path.join(ROOT, "examples", "probability_maps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.days, args.every, args.seed) == (20, 7, 36, 0)
    args = mod.parse(["--members", "64", "--days", "2", "--every", "9", "--seed", "3"])
    assert (args.members, args.days, args.every, args.seed) == (64, 2, 9, 3)
    entries = mod.entries()
    assert [e[:3] for e in entries] == [("precnv", 0, "prob_above"), ("z_plev", 0, "quantile"), ("z_plev", 0, "quantile"),
                                        ("z_plev", 0, "quantile"), ("t_grid", 7, "min")]
    assert [e[3] for e in entries[1:4]] == [0.1, 0.5, 0.9] and abs(entries[0][3] * 86400.0 - 1000.0) < 1e-9
    for bad in (["--members", "1"], ["--members", "65"], ["--days", "0"], ["--every", "0"]):
        with pytest.raises(SystemExit):
            mod.parse(bad)
