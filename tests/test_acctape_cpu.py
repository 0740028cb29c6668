"""CPU tier: the accumulation tape's entry points (spd_model_acctape_*) are declared, exported and bound; the argument checks the
library makes before it needs a model or a device, in their documented order; the daily-precipitation example parses its
arguments."""
import ctypes as C
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCTAPE_SYMBOLS = ("spd_model_acctape_configure", "spd_model_acctape_reset", "spd_model_acctape_info", "spd_model_acctape_times",
                   "spd_model_acctape_read")
SUM, MEAN, MIN, MAX = 0, 1, 2, 3


def test_acctape_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in ACCTAPE_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for op, value in (("SPD_ACC_SUM", SUM), ("SPD_ACC_MEAN", MEAN), ("SPD_ACC_MIN", MIN), ("SPD_ACC_MAX", MAX)):
        assert "#define %s %d" % (op, value) in header
        assert "%s = %d" % (op, value) in fortran
        assert getattr(L, op) == value
    for method in ("acctape_configure", "acctape_reset", "acctape_info", "acctape_steps", "acctape_times", "acctape_counts", "acctape"):
        assert hasattr(EnsembleModel, method), method
    assert EnsembleModel.ACCTAPE_OPS == dict(sum=SUM, mean=MEAN, min=MIN, max=MAX)
    assert len(EnsembleModel.ACCTAPE_NAMES) == 14 and set(EnsembleModel.ACCTAPE_THREE_PLANES) < set(EnsembleModel.ACCTAPE_NAMES)


def _entries(*pairs):
    names = (C.c_char_p * max(len(pairs), 1))(*[n.encode() for n, _ in pairs])
    ops = (C.c_int * max(len(pairs), 1))(*[op for _, op in pairs])
    return names, ops, len(pairs)


@pytest.mark.parametrize("pairs, every, capacity, dtype, message", [
    ((("precnv", SUM), ("t_grid", SUM)), 36, 4, 0, b"unknown variable 't_grid'"),
    ((("hfluxn", MEAN),), 36, 4, 0, b"'hfluxn' is not stored in every plane on every step"),
    ((("qcloud_equiv", MEAN),), 36, 4, 0, b"'qcloud_equiv' is not stored in every plane on every step"),
    ((("olr", 4),), 36, 4, 0, b"unknown op 4 for 'olr'"),
    ((("olr", -1),), 36, 4, 0, b"unknown op -1 for 'olr'"),
    ((("olr", MEAN), ("shf", MAX), ("olr", MEAN)), 36, 4, 0, b"('olr', 1) named twice"),
    ((("precnv", SUM),), 0, 4, 0, b"every must be at least 1"),
    ((("precnv", SUM),), 36, 0, 0, b"capacity must be at least 1"),
    ((("precnv", SUM),), 36, 4, 2, b"dtype must be SPD_TAPE_F32 or SPD_TAPE_F64"),
    ((("precnv", SUM), ("precnv", MAX), ("slru", MIN)), 36, 4, 1, b"null model"),  # (a name under two ops is two entries)
])
def test_configure_checks_its_arguments_first(hip_lib, pairs, every, capacity, dtype, message):
    names, ops, n = _entries(*pairs)
    rc = hip_lib.spd_model_acctape_configure(None, names, ops, n, every, capacity, dtype)
    assert rc == -1
    assert message in hip_lib.spd_last_error(), hip_lib.spd_last_error()
    assert b"spd_model_acctape_configure" in hip_lib.spd_last_error()


def test_argument_checks_come_in_the_documented_order(hip_lib):
    """unknown name, unknown op, entry twice, every, capacity, dtype, then the null model"""
    cases = [((("t_grid", 9), ("t_grid", 9)), 0, 0, 7, b"unknown variable"), ((("olr", 9), ("olr", 9)), 0, 0, 7, b"unknown op"),
             ((("olr", MIN), ("olr", MIN)), 0, 0, 7, b"named twice"), ((("olr", MIN),), 0, 0, 7, b"every must"),
             ((("olr", MIN),), 1, 0, 7, b"capacity must"), ((("olr", MIN),), 1, 1, 7, b"dtype must"),
             ((("olr", MIN),), 1, 1, 1, b"null model")]
    for pairs, every, capacity, dtype, message in cases:
        names, ops, n = _entries(*pairs)
        assert hip_lib.spd_model_acctape_configure(None, names, ops, n, every, capacity, dtype) == -1
        assert message in hip_lib.spd_last_error(), (message, hip_lib.spd_last_error())


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    buf = C.c_double()
    taken, held = C.c_longlong(), C.c_int()
    rows = (C.c_int32 * 7)()
    assert hip_lib.spd_model_acctape_configure(None, None, None, -1, 36, 4, 0) == -1
    assert b"spd_model_acctape_configure" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_acctape_configure(None, None, None, 1, 36, 4, 0) == -1
    assert b"spd_model_acctape_configure: bad list of entries" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_acctape_configure(None, None, None, 0, 36, 4, 0) == -1  # (switching off still needs a model)
    assert b"spd_model_acctape_configure: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_acctape_reset(None) == -1 and b"spd_model_acctape_reset" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_acctape_info(None, C.byref(taken), C.byref(held), None, None, None) == -1
    assert b"spd_model_acctape_info" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_acctape_times(None, rows, 1) == -1 and b"spd_model_acctape_times" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_acctape_read(None, b"olr", MEAN, 0, 1, 0, 1, C.byref(buf), 8, None) == -1
    assert b"spd_model_acctape_read" in hip_lib.spd_last_error()


def test_daily_precipitation_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("daily_precipitation", os.path.join(ROOT, "examples", "daily_precipitation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.days, args.call_days, args.start, args.noise) == (16, 10, 5, "1982-01", 0.01)
    args = mod.parse(["--members", "64", "--days", "30", "--call-days", "3", "--start", "1983-06", "--noise", "0.1"])
    assert (args.members, args.days, args.call_days, args.start, args.noise) == (64, 30, 3, "1983-06", 0.1)
    assert mod.EVERY == 36 and mod.STEP_SECONDS == 2400.0
    assert mod.ENTRIES == (("precnv", "sum"), ("precls", "sum"), ("precnv", "max"), ("olr", "mean"), ("tsr", "mean"))
    with pytest.raises(SystemExit):
        mod.parse(["--members", "1"])
    with pytest.raises(SystemExit):
        mod.parse(["--days", "0"])
