"""CPU tier: the window tape's entry points (spd_model_wintape_*, spd_wintape_plan) are declared, exported and bound; the argument
checks the library makes before it needs a model or a device, in their documented order; the recorder's schedule
(spd_wintape_plan, the code the step loop takes its decisions from) against Python's datetime, whose calendar agrees with the
model's (leap when year % 4 == 0) for 1901 ... 2099; the monthly-climate example parses its arguments."""
import ctypes as C
import importlib.util
import os
from datetime import datetime, timedelta

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINTAPE_SYMBOLS = ("spd_model_wintape_configure", "spd_model_wintape_reset", "spd_model_wintape_info", "spd_model_wintape_times",
                   "spd_model_wintape_read", "spd_wintape_plan")
SUM, MEAN, MIN, MAX, ABOVE, BELOW = 0, 1, 2, 3, 4, 5
STEPS, DAY, MONTH = 0, 1, 2
SIXTEEN = (b"(u_grid, v_grid, t_grid, q_grid, phi_grid, ps_grid, precnv, precls, u_plev, v_plev, t_plev, q_plev, z_plev, mslp, "
           b"wspd_grid, wspd_plev)")


def test_wintape_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in WINTAPE_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    constants = (("SPD_WIN_SUM", SUM), ("SPD_WIN_MEAN", MEAN), ("SPD_WIN_MIN", MIN), ("SPD_WIN_MAX", MAX), ("SPD_WIN_COUNT_ABOVE", ABOVE),
                 ("SPD_WIN_COUNT_BELOW", BELOW), ("SPD_WINDOW_STEPS", STEPS), ("SPD_WINDOW_DAY", DAY), ("SPD_WINDOW_MONTH", MONTH))
    for name, value in constants:
        assert "#define %s %d" % (name, value) in header
        assert "%s = %d" % (name, value) in fortran
        assert getattr(L, name) == value
    for op in ("SUM", "MEAN", "MIN", "MAX"):  # (the numbers of SPD_ACC_*)
        assert getattr(L, "SPD_WIN_" + op) == getattr(L, "SPD_ACC_" + op)
    for method in ("wintape_configure", "wintape_reset", "wintape_info", "wintape_steps", "wintape_times", "wintape_counts", "wintape",
                   "wintape_plan"):
        assert hasattr(EnsembleModel, method), method
    assert EnsembleModel.WINTAPE_OPS == dict(sum=SUM, mean=MEAN, min=MIN, max=MAX, count_above=ABOVE, count_below=BELOW)
    assert EnsembleModel.WINTAPE_NAMES == EnsembleModel.STATS_VARIABLES + ("wspd_grid", "wspd_plev")
    assert len(EnsembleModel.WINTAPE_NAMES) == 16


def _entries(*triples):
    """(name, op[, threshold]) -> the three C arrays and their length (thresholds: None when no entry gives one)"""
    n = max(len(triples), 1)
    names = (C.c_char_p * n)(*[t[0].encode() for t in triples])
    ops = (C.c_int * n)(*[t[1] for t in triples])
    thresholds = None
    if any(len(t) > 2 for t in triples):
        thresholds = (C.c_double * n)(*[t[2] if len(t) > 2 else 0.0 for t in triples])
    return names, ops, thresholds, len(triples)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("triples, window, every, sample_every, capacity, dtype, message", [
    ((("t_grid", MEAN), ("olr", MEAN)), STEPS, 36, 1, 4, 0, b"unknown variable 'olr' " + SIXTEEN),
    ((("wspd", MAX),), STEPS, 36, 1, 4, 0, b"unknown variable 'wspd' " + SIXTEEN),
    ((("t_grid", 6),), STEPS, 36, 1, 4, 0, b"unknown op 6 for 't_grid'"),
    ((("wspd_grid", -1),), STEPS, 36, 1, 4, 0, b"unknown op -1 for 'wspd_grid'"),
    ((("t_grid", BELOW),), STEPS, 36, 1, 4, 0, b"SPD_WIN_COUNT_BELOW of 't_grid' needs a finite threshold"),  # (no thresholds at all)
    ((("t_grid", MEAN, 0.0), ("t_grid", ABOVE, NAN)), STEPS, 36, 1, 4, 0, b"SPD_WIN_COUNT_ABOVE of 't_grid' needs a finite threshold"),
    ((("mslp", BELOW, -INF),), STEPS, 36, 1, 4, 0, b"SPD_WIN_COUNT_BELOW of 'mslp' needs a finite threshold"),
    ((("t_grid", MEAN), ("mslp", MAX), ("t_grid", MEAN)), STEPS, 36, 1, 4, 0, b"('t_grid', 1) named twice"),
    ((("t_grid", BELOW, 273.15), ("t_grid", BELOW, 250.0)), STEPS, 36, 1, 4, 0, b"('t_grid', 5) named twice"),
    ((("t_grid", MEAN),), 3, 0, 1, 4, 0, b"unknown window kind 3"),
    ((("t_grid", MEAN),), -1, 0, 1, 4, 0, b"unknown window kind -1"),
    ((("t_grid", MEAN),), STEPS, 0, 1, 4, 0, b"every must be at least 1 for SPD_WINDOW_STEPS"),
    ((("t_grid", MEAN),), DAY, 36, 1, 4, 0, b"every must be 0 for SPD_WINDOW_DAY and SPD_WINDOW_MONTH"),
    ((("t_grid", MEAN),), MONTH, 1, 1, 4, 0, b"every must be 0 for SPD_WINDOW_DAY and SPD_WINDOW_MONTH"),
    ((("t_grid", MEAN),), MONTH, 0, 0, 4, 0, b"sample_every must be at least 1"),
    ((("t_grid", MEAN),), DAY, 0, 9, 0, 0, b"capacity must be at least 1"),
    ((("t_grid", MEAN),), DAY, 0, 9, 4, 2, b"dtype must be SPD_TAPE_F32 or SPD_TAPE_F64"),
    # (a name under several ops is several entries; above and below of one name are two)
    ((("t_grid", MEAN), ("t_grid", MAX), ("t_grid", ABOVE, 300.0), ("t_grid", BELOW, 273.15), ("wspd_plev", MAX)), MONTH, 0, 9, 4, 1,
     b"null model"),
])
def test_configure_checks_its_arguments_first(hip_lib, triples, window, every, sample_every, capacity, dtype, message):
    names, ops, thresholds, n = _entries(*triples)
    rc = hip_lib.spd_model_wintape_configure(None, names, ops, thresholds, n, window, every, sample_every, capacity, dtype)
    assert rc == -1
    assert message in hip_lib.spd_last_error(), hip_lib.spd_last_error()
    assert b"spd_model_wintape_configure" in hip_lib.spd_last_error()


def test_argument_checks_come_in_the_documented_order(hip_lib):
    """bad list, unknown name, unknown op, count op without a finite threshold, entry twice, window kind, every, sample_every,
    capacity, dtype, then the null model: each case is wrong in everything that comes later as well."""
    twice = lambda *t: (t, t)  # noqa: E731
    cases = [(twice("olr", 9), 7, -1, 0, 0, 7, b"unknown variable"),
             ((("t_grid", ABOVE, NAN), ("t_grid", 9, NAN)), 7, -1, 0, 0, 7, b"unknown op"),
             (twice("t_grid", ABOVE, NAN), 7, -1, 0, 0, 7, b"needs a finite threshold"),
             (twice("t_grid", ABOVE, 1.0), 7, -1, 0, 0, 7, b"named twice"),
             ((("t_grid", ABOVE, 1.0),), 7, -1, 0, 0, 7, b"unknown window kind"),
             ((("t_grid", ABOVE, 1.0),), STEPS, 0, 0, 0, 7, b"every must be at least 1"),
             ((("t_grid", ABOVE, 1.0),), DAY, 5, 0, 0, 7, b"every must be 0"),
             ((("t_grid", ABOVE, 1.0),), DAY, 0, 0, 0, 7, b"sample_every must"),
             ((("t_grid", ABOVE, 1.0),), DAY, 0, 1, 0, 7, b"capacity must"),
             ((("t_grid", ABOVE, 1.0),), DAY, 0, 1, 1, 7, b"dtype must"),
             ((("t_grid", ABOVE, 1.0),), DAY, 0, 1, 1, 1, b"null model")]
    for triples, window, every, sample_every, capacity, dtype, message in cases:
        names, ops, thresholds, n = _entries(*triples)
        assert hip_lib.spd_model_wintape_configure(None, names, ops, thresholds, n, window, every, sample_every, capacity, dtype) == -1
        assert message in hip_lib.spd_last_error(), (message, hip_lib.spd_last_error())
    # the list itself comes before everything else
    assert hip_lib.spd_model_wintape_configure(None, None, None, None, 2, 7, -1, 0, 0, 7) == -1
    assert b"bad list of entries" in hip_lib.spd_last_error()


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    buf = C.c_double()
    taken, held = C.c_longlong(), C.c_int()
    rows = (C.c_int32 * 8)()
    assert hip_lib.spd_model_wintape_configure(None, None, None, None, -1, STEPS, 36, 1, 4, 0) == -1
    assert b"spd_model_wintape_configure: bad list of entries" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_wintape_configure(None, None, None, None, 1, STEPS, 36, 1, 4, 0) == -1
    assert b"spd_model_wintape_configure: bad list of entries" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_wintape_configure(None, None, None, None, 0, STEPS, 36, 1, 4, 0) == -1  # (switching off still needs a model)
    assert b"spd_model_wintape_configure: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_wintape_reset(None) == -1 and b"spd_model_wintape_reset" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_wintape_info(None, C.byref(taken), C.byref(held), None, None, None, None, None) == -1
    assert b"spd_model_wintape_info" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_wintape_times(None, rows, 1) == -1 and b"spd_model_wintape_times" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_wintape_read(None, b"t_grid", MEAN, 0, 1, 0, 1, C.byref(buf), 8, None) == -1
    assert b"spd_model_wintape_read" in hip_lib.spd_last_error()


# ---- the schedule ------------------------------------------------------------------------------------------------------
def plan(hip_lib, start, step0, nsteps, window, every, sample_every, max_rows=64):
    rows = np.zeros((max_rows, 8), dtype=np.int32)
    n = hip_lib.spd_wintape_plan(start.year, start.month, start.day, start.hour, start.minute, step0, nsteps, window, every,
                                 sample_every, rows.ctypes.data_as(C.POINTER(C.c_int32)), max_rows)
    assert 0 <= n <= max_rows, hip_lib.spd_last_error()
    return rows[:n].tolist()


def by_datetime(start, step0, nsteps, window, every, sample_every):
    """the same rows from Python's calendar: a loop over the steps with the definition's two rules"""
    rows, first, samples = [], step0, 0
    for k in range(step0 + 1, step0 + nsteps + 1):
        now = start + timedelta(minutes=40 * (k - step0))
        samples += 1 if k % sample_every == 0 else 0
        midnight = (now.hour, now.minute) == (0, 0)
        if k % every == 0 if window == STEPS else midnight and (window == DAY or now.day == 1):
            rows.append([k, now.year, now.month, now.day, now.hour, now.minute, samples, k - first])
            first, samples = k, 0
    return rows


def test_month_windows_over_a_28_day_february(hip_lib):
    start = datetime(1982, 1, 31, 12, 0)
    rows = plan(hip_lib, start, 0, 1062, MONTH, 0, 9)
    assert rows == [[18, 1982, 2, 1, 0, 0, 2, 18], [1026, 1982, 3, 1, 0, 0, 112, 1008]]
    assert rows == by_datetime(start, 0, 1062, MONTH, 0, 9)


def test_month_window_over_the_leap_day(hip_lib):
    start = datetime(1980, 2, 28, 0, 0)
    rows = plan(hip_lib, start, 0, 80, MONTH, 0, 1)
    assert rows == [[72, 1980, 3, 1, 0, 0, 72, 72]]
    assert rows == by_datetime(start, 0, 80, MONTH, 0, 1)
    # ... and no leap day in 1982: the month ends a day earlier
    assert plan(hip_lib, datetime(1982, 2, 28, 0, 0), 0, 80, MONTH, 0, 1) == [[36, 1982, 3, 1, 0, 0, 36, 36]]


def test_month_window_over_the_year_end(hip_lib):
    start = datetime(1982, 12, 31, 0, 0)
    rows = plan(hip_lib, start, 0, 40, MONTH, 0, 1)
    assert rows == [[36, 1983, 1, 1, 0, 0, 36, 36]]
    assert rows == by_datetime(start, 0, 40, MONTH, 0, 1)


def test_day_windows_with_an_empty_first_one(hip_lib):
    start = datetime(1982, 1, 31, 12, 0)
    rows = plan(hip_lib, start, 0, 100, DAY, 0, 36)
    assert [r[0] for r in rows] == [18, 54, 90]
    assert [r[6] for r in rows] == [0, 1, 1] and [r[7] for r in rows] == [18, 36, 36]
    assert rows == by_datetime(start, 0, 100, DAY, 0, 36)


def test_step_windows_against_a_three_line_loop(hip_lib):
    start, step0, nsteps, every, sample_every = datetime(1982, 1, 1), 2, 23, 4, 3
    rows = plan(hip_lib, start, step0, nsteps, STEPS, every, sample_every)
    closes = [k for k in range(step0 + 1, step0 + nsteps + 1) if k % every == 0]
    edges = [step0] + closes
    samples = [sum(1 for k in range(a + 1, b + 1) if k % sample_every == 0) for a, b in zip(edges[:-1], edges[1:])]
    assert [r[0] for r in rows] == closes == [4, 8, 12, 16, 20, 24]
    assert [r[6] for r in rows] == samples == [1, 1, 2, 1, 1, 2]
    assert [r[7] for r in rows] == [2, 4, 4, 4, 4, 4]
    assert rows == by_datetime(start, step0, nsteps, STEPS, every, sample_every)


def test_a_year_of_months_and_days_against_datetime(hip_lib):
    """every month end and every midnight of the leap year 1984 and of 1985, from mid-month"""
    start = datetime(1984, 1, 15, 8, 0)
    nsteps = 36 * 700
    months = plan(hip_lib, start, 5, nsteps, MONTH, 0, 7)
    assert len(months) == 23 and months == by_datetime(start, 5, nsteps, MONTH, 0, 7)
    days = plan(hip_lib, start, 5, nsteps, DAY, 0, 7, max_rows=800)
    assert len(days) == 700 and days == by_datetime(start, 5, nsteps, DAY, 0, 7)


def test_plan_counts_beyond_the_rows_it_may_write_and_checks_its_arguments(hip_lib):
    rows = np.full((2, 8), -7, dtype=np.int32)
    ptr = rows.ctypes.data_as(C.POINTER(C.c_int32))
    assert hip_lib.spd_wintape_plan(1982, 1, 1, 0, 0, 0, 100, STEPS, 10, 1, ptr, 1) == 10
    assert rows[0].tolist() == [10, 1982, 1, 1, 6, 40, 10, 10] and rows[1].tolist() == [-7] * 8
    assert hip_lib.spd_wintape_plan(1982, 1, 1, 0, 0, 0, 100, STEPS, 10, 1, None, 0) == 10
    for args, message in (((1982, 13, 1, 0, 0, 0, 10, STEPS, 1, 1), b"bad date"), ((1982, 1, 1, 0, 0, -1, 10, STEPS, 1, 1), b"negative"),
                          ((1982, 1, 1, 0, 0, 0, 10, 3, 1, 1), b"unknown window kind"), ((1982, 1, 1, 0, 0, 0, 10, STEPS, 0, 1), b"every must"),
                          ((1982, 1, 1, 0, 0, 0, 10, MONTH, 2, 1), b"every must be 0"), ((1982, 1, 1, 0, 0, 0, 10, DAY, 0, 0), b"sample_every must")):
        assert hip_lib.spd_wintape_plan(*args, ptr, 2) == -1
        assert b"spd_wintape_plan" in hip_lib.spd_last_error() and message in hip_lib.spd_last_error(), hip_lib.spd_last_error()
    assert hip_lib.spd_wintape_plan(1982, 1, 1, 0, 0, 0, 10, STEPS, 1, 1, None, 2) == -1 and b"bad destination" in hip_lib.spd_last_error()


def test_the_python_plan_is_the_library_s(hip_lib):
    import pyspeedy_amd
    start = datetime(1982, 1, 31, 12, 0)
    assert pyspeedy_amd.wintape_plan(start, 0, 1062, "month", sample_every=9).tolist() == plan(hip_lib, start, 0, 1062, MONTH, 0, 9)
    assert pyspeedy_amd.wintape_plan((1982, 1, 31, 12, 0), 0, 100, "day", 36).tolist() == plan(hip_lib, start, 0, 100, DAY, 0, 36)
    assert pyspeedy_amd.wintape_plan(start, 2, 23, 4, 3).tolist() == plan(hip_lib, start, 2, 23, STEPS, 4, 3)
    assert pyspeedy_amd.wintape_plan(start, 0, 5, "day").shape == (0, 8)
    with pytest.raises(ValueError, match="window must be"):
        pyspeedy_amd.wintape_plan(start, 0, 5, "week")


def test_monthly_climate_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("monthly_climate", os.path.join(ROOT, "examples", "monthly_climate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.months, args.call_days, args.start, args.noise) == (16, 2, 5, "1982-01", 0.01)
    args = mod.parse(["--members", "64", "--months", "12", "--call-days", "7", "--start", "1984-02", "--noise", "0.1"])
    assert (args.members, args.months, args.call_days, args.start, args.noise) == (64, 12, 7, "1984-02", 0.1)
    assert mod.SAMPLE_EVERY == 9 and mod.FREEZING == 273.15 and mod.LEVELS_HPA == (500.0,)
    assert mod.ENTRIES == (("z_plev", "mean"), ("mslp", "mean"), ("wspd_grid", "max"), ("t_grid", "min"), ("t_grid", "max"),
                           ("t_grid", "count_below", 273.15))
    assert mod.days_of(1982, 1, 2) == 59 and mod.days_of(1984, 2, 1) == 29 and mod.days_of(1982, 12, 2) == 62
    with pytest.raises(SystemExit):
        mod.parse(["--members", "1"])
    with pytest.raises(SystemExit):
        mod.parse(["--months", "0"])
