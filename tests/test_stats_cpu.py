"""CPU tier: the time-statistics entry points (spd_model_stats_*) are declared, exported and bound; the argument checks the
library makes before it needs a model or a device; the climate-means example parses its arguments."""
import ctypes as C
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_SYMBOLS = ("spd_model_stats_configure", "spd_model_stats_reset", "spd_model_stats_samples", "spd_model_stats_read",
                 "spd_model_stats_ensemble")


def test_stats_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd._lib as L
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in STATS_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for kind, value in (("SPD_STATS_MEAN", 0), ("SPD_STATS_VARIANCE", 1), ("SPD_STATS_STD", 2)):
        assert "#define %s %d" % (kind, value) in header
        assert getattr(L, kind) == value


def _names(*names):
    return (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])


@pytest.mark.parametrize("names, every, message", [
    (("t_grid", "olr"), 9, b"unknown variable 'olr'"),
    (("t_grid", "t_grid"), 9, b"named twice"),
    (("precnv",), 0, b"every must be at least 1"),
    (("ps_grid",), 9, b"null model"),
])
def test_configure_checks_its_arguments_first(hip_lib, names, every, message):
    rc = hip_lib.spd_model_stats_configure(None, _names(*names), len(names), every, 1)
    assert rc == -1
    assert message in hip_lib.spd_last_error()


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    buf = C.c_double()
    assert hip_lib.spd_model_stats_configure(None, None, -1, 9, 1) == -1
    assert hip_lib.spd_model_stats_reset(None) == -1 and b"spd_model_stats_reset" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_stats_samples(None) == -1 and b"spd_model_stats_samples" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_stats_read(None, b"t_grid", 0, 0, 1, C.byref(buf), 8, None) == -1
    assert b"spd_model_stats_read" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_stats_ensemble(None, b"t_grid", 2, C.byref(buf), 8, None) == -1
    assert b"spd_model_stats_ensemble" in hip_lib.spd_last_error()


def test_climate_means_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("climate_means", os.path.join(ROOT, "examples", "climate_means.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.months, args.every, args.start) == (16, 2, 9, "1982-01")
    args = mod.parse(["--members", "64", "--months", "12", "--every", "36", "--start", "1983-06", "--noise", "0.1"])
    assert (args.members, args.months, args.every, args.start, args.noise) == (64, 12, 36, "1983-06", 0.1)
    with pytest.raises(SystemExit):
        mod.parse(["--every", "0"])
    with pytest.raises(SystemExit):
        mod.parse(["--members", "1"])
