"""CPU tier: the tape's entry points (spd_model_tape_*) are declared, exported and bound; the argument checks the library makes
before it needs a model or a device; the six-hourly-series example parses its arguments."""
import ctypes as C
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPE_SYMBOLS = ("spd_model_tape_configure", "spd_model_tape_reset", "spd_model_tape_info", "spd_model_tape_times",
                "spd_model_tape_read")


def test_tape_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd._lib as L
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in TAPE_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for kind, value in (("SPD_TAPE_F32", 0), ("SPD_TAPE_F64", 1)):
        assert "#define %s %d" % (kind, value) in header
        assert getattr(L, kind) == value


def _names(*names):
    return (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])


@pytest.mark.parametrize("names, every, capacity, dtype, message", [
    (("t_grid", "olr"), 9, 4, 0, b"unknown variable 'olr'"),
    (("t_grid", "t_grid"), 9, 4, 0, b"named twice"),
    (("precnv",), 0, 4, 0, b"every must be at least 1"),
    (("precnv",), 9, 0, 0, b"capacity must be at least 1"),
    (("mslp",), 9, 4, 2, b"dtype must be SPD_TAPE_F32 or SPD_TAPE_F64"),
    (("mslp",), 9, 4, -1, b"dtype must be SPD_TAPE_F32 or SPD_TAPE_F64"),
    (("ps_grid",), 9, 4, 1, b"null model"),
])
def test_configure_checks_its_arguments_first(hip_lib, names, every, capacity, dtype, message):
    rc = hip_lib.spd_model_tape_configure(None, _names(*names), len(names), every, capacity, dtype)
    assert rc == -1
    assert message in hip_lib.spd_last_error()
    assert b"spd_model_tape_configure" in hip_lib.spd_last_error()


def test_argument_checks_come_in_the_documented_order(hip_lib):
    """unknown name, name twice, every, capacity, dtype, then the null model"""
    cases = [(("olr", "olr"), 0, 0, 7, b"unknown variable"), (("mslp", "mslp"), 0, 0, 7, b"named twice"),
             (("mslp",), 0, 0, 7, b"every must"), (("mslp",), 1, 0, 7, b"capacity must"), (("mslp",), 1, 1, 7, b"dtype must"),
             (("mslp",), 1, 1, 1, b"null model")]
    for names, every, capacity, dtype, message in cases:
        assert hip_lib.spd_model_tape_configure(None, _names(*names), len(names), every, capacity, dtype) == -1
        assert message in hip_lib.spd_last_error(), (message, hip_lib.spd_last_error())


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    buf = C.c_double()
    taken, held = C.c_longlong(), C.c_int()
    rows = (C.c_int32 * 6)()
    assert hip_lib.spd_model_tape_configure(None, None, -1, 9, 4, 0) == -1
    assert b"spd_model_tape_configure" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tape_configure(None, None, 0, 9, 4, 0) == -1  # (switching off still needs a model)
    assert b"spd_model_tape_configure: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tape_reset(None) == -1 and b"spd_model_tape_reset" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tape_info(None, C.byref(taken), C.byref(held), None, None, None) == -1
    assert b"spd_model_tape_info" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tape_times(None, rows, 1) == -1 and b"spd_model_tape_times" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tape_read(None, b"t_grid", 0, 1, 0, 1, C.byref(buf), 8, None) == -1
    assert b"spd_model_tape_read" in hip_lib.spd_last_error()


def test_six_hourly_series_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("six_hourly_series", os.path.join(ROOT, "examples", "six_hourly_series.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.days, args.call_days, args.start, args.noise, args.dtype) == (16, 30, 1, "1982-01", 0.01, "float32")
    args = mod.parse(["--members", "64", "--days", "10", "--call-days", "5", "--start", "1983-06", "--noise", "0.1", "--dtype", "float64"])
    assert (args.members, args.days, args.call_days, args.start, args.noise, args.dtype) == (64, 10, 5, "1983-06", 0.1, "float64")
    with pytest.raises(SystemExit):
        mod.parse(["--members", "1"])
    with pytest.raises(SystemExit):
        mod.parse(["--days", "0"])
    with pytest.raises(SystemExit):
        mod.parse(["--dtype", "float16"])
