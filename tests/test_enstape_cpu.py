"""CPU tier: the ensemble tape's entry points (spd_model_enstape_*) are declared, exported and bound; the argument checks the
library makes before it needs a model or a device, in their documented order; merge_moments against numpy; the
ensemble-spread-series example parses its arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENSTAPE_SYMBOLS = ("spd_model_enstape_configure", "spd_model_enstape_reset", "spd_model_enstape_info", "spd_model_enstape_times",
                   "spd_model_enstape_read")
EPS = 2.0 ** -52


def test_enstape_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd._lib as L
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in ENSTAPE_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for kind, value in (("SPD_ENS_MEAN", 0), ("SPD_ENS_STD", 1), ("SPD_ENS_M2", 2)):
        assert "#define %s %d" % (kind, value) in header
        assert "%s = %d" % (kind, value) in fortran
        assert getattr(L, kind) == value


def _names(*names):
    return (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])


@pytest.mark.parametrize("names, every, capacity, message", [
    (("t_grid", "olr"), 9, 4, b"unknown variable 'olr'"),
    (("t_grid", "t_grid"), 9, 4, b"named twice"),
    (("precnv",), 0, 4, b"every must be at least 1"),
    (("precnv",), 9, 0, b"capacity must be at least 1"),
    (("ps_grid",), 9, 4, b"null model"),
])
def test_configure_checks_its_arguments_first(hip_lib, names, every, capacity, message):
    rc = hip_lib.spd_model_enstape_configure(None, _names(*names), len(names), every, capacity)
    assert rc == -1
    assert message in hip_lib.spd_last_error()
    assert b"spd_model_enstape_configure" in hip_lib.spd_last_error()


def test_argument_checks_come_in_the_documented_order(hip_lib):
    """unknown name, name twice, every, capacity, then the null model"""
    cases = [(("olr", "olr"), 0, 0, b"unknown variable"), (("mslp", "mslp"), 0, 0, b"named twice"),
             (("mslp",), 0, 0, b"every must"), (("mslp",), 1, 0, b"capacity must"), (("mslp",), 1, 1, b"null model")]
    for names, every, capacity, message in cases:
        assert hip_lib.spd_model_enstape_configure(None, _names(*names), len(names), every, capacity) == -1
        assert message in hip_lib.spd_last_error(), (message, hip_lib.spd_last_error())


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    buf = C.c_double()
    taken, held = C.c_longlong(), C.c_int()
    rows = (C.c_int32 * 6)()
    assert hip_lib.spd_model_enstape_configure(None, None, -1, 9, 4) == -1
    assert b"spd_model_enstape_configure" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_enstape_configure(None, None, 0, 9, 4) == -1  # (switching off still needs a model)
    assert b"spd_model_enstape_configure: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_enstape_reset(None) == -1 and b"spd_model_enstape_reset" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_enstape_info(None, C.byref(taken), C.byref(held), None, None, None) == -1
    assert b"spd_model_enstape_info" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_enstape_times(None, rows, 1) == -1 and b"spd_model_enstape_times" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_enstape_read(None, b"t_grid", 0, 0, 1, C.byref(buf), 8, None) == -1
    assert b"spd_model_enstape_read" in hip_lib.spd_last_error()


def _moments(x):
    import torch
    mean = x.mean(axis=0)
    return x.shape[0], torch.from_numpy(mean), torch.from_numpy(((x - mean) ** 2).sum(axis=0))


@pytest.mark.parametrize("offset", [0.0, 250.0, 1.0e5])
def test_merge_moments_against_numpy(offset):
    """Random fp64 data of 23 members split into uneven parts -- one of a single member, an empty entry with n = 0 in the
    middle -- merged with Chan's formula: within the bounds the GPU tier holds the kernels to (N eps kappa in pointwise form,
    with the factor for the reference's own rounding), against numpy's mean and std(ddof=1)."""
    import torch
    from pyspeedy_amd.ensemble import merge_moments
    M = 23
    x = offset + np.random.default_rng(7).normal(0.0, 1.0, (M, 5, 48, 96))
    cuts = [0, 9, 10, 10, 17, 23]  # parts of 9, 1, 0, 7 and 6 members
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.append((0, torch.zeros(5, 48, 96, dtype=torch.float64), torch.zeros(5, 48, 96, dtype=torch.float64)) if a == b
                     else _moments(x[a:b]))
    assert [p[0] for p in parts] == [9, 1, 0, 7, 6]
    n, mean, std = merge_moments(parts)
    assert n == M and mean.dtype == torch.float64 and std.dtype == torch.float64
    ref_mean, ref_var = x.mean(axis=0), x.var(axis=0, ddof=1)
    assert (np.abs(mean.numpy() - ref_mean) <= 4 * M * EPS * np.abs(x).max(axis=0)).all()
    v = std.numpy() ** 2
    bound = 16 * M * EPS * (ref_var + np.abs(ref_mean) * np.sqrt(ref_var))
    assert (np.abs(v - ref_var) <= bound).all(), float((np.abs(v - ref_var) / bound).max())
    assert np.abs(std.numpy() - x.std(axis=0, ddof=1)).max() <= float(np.sqrt(bound).max())
    # one part is that part; ddof = 0 is the population's; a single member has no spread to give
    n1, mean1, std1 = merge_moments(parts[:1], ddof=0)
    assert n1 == 9 and torch.equal(mean1, parts[0][1]) and torch.equal(std1, torch.sqrt(parts[0][2] / 9))
    n1, mean1, std1 = merge_moments([parts[1]])
    assert n1 == 1 and torch.equal(mean1, torch.from_numpy(x[9])) and bool(torch.isnan(std1).all())
    with pytest.raises(ValueError):
        merge_moments([parts[2]])


def test_ensemble_spread_series_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("ensemble_spread_series", os.path.join(ROOT, "examples", "ensemble_spread_series.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.days, args.call_days, args.start, args.noise, args.block_members) == (64, 30, 5, "1982-01", 0.01, 0)
    args = mod.parse(["--members", "1024", "--days", "10", "--call-days", "2", "--start", "1983-06", "--noise", "0.1",
                      "--block-members", "32"])
    assert (args.members, args.days, args.call_days, args.start, args.noise, args.block_members) == (1024, 10, 2, "1983-06", 0.1, 32)
    assert mod.NAMES == ("z_plev", "mslp") and mod.EVERY == 9
    with pytest.raises(SystemExit):
        mod.parse(["--members", "1"])
    with pytest.raises(SystemExit):
        mod.parse(["--days", "0"])
    with pytest.raises(SystemExit):
        mod.parse(["--block-members", "-1"])
