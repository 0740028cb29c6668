"""CPU tier: the definition of the spectra pinned to the reference's transforms through the arbiter
(tests/spectra_reference.py) on the golden states; the truncation the kernel relies on; the entry points (spd_model_spectra_*) are
declared, exported and bound; the argument checks the library makes before it needs a model or a device; the example parses its
arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import spectra_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECTRA_SYMBOLS = ("spd_model_spectra_configure", "spd_model_spectra_reset", "spd_model_spectra_info", "spd_model_spectra_times",
                   "spd_model_spectra_read", "spd_model_spectra_compute")


@pytest.fixture(scope="module")
def run(golden_dir):
    return np.load(os.path.join(golden_dir, "run.npz"))


@pytest.mark.parametrize("time_level", [0, 1])
def test_normalisation_against_the_reference_transforms(oracle, run, time_level):
    """On d3 of the golden run, levels 0, 3 and 7: the sum over l of the rotational and divergent spectra against the Gaussian-
    weighted area mean of (u^2 + v^2) / 2 from the oracle's vort2vel + spec2grid(kcos = 2); the sum over l >= 1 of t_spectrum against
    the area variance of T; t_mean against the area mean of T.  Measured relative differences: kinetic energy 1.7e-5 ... 5.2e-5
    (bound 2e-4), T variance <= 5.3e-4 (bound 2e-3), T mean <= 5e-6 (bound 2e-5) -- the reference's approximate Gaussian latitudes
    and fp32 constants, not round-off; a wrong w_m or factor would show as sqrt(2) or 2."""
    wt, elm2 = oracle.table("wt"), oracle.table("elm2")
    state = {n: run["d3_" + n][..., time_level] for n in ("vor", "div", "t", "tr", "ps")}
    got = ref.spectra(state["vor"], state["div"], state["t"], state["tr"], state["ps"], elm2)
    for k in (0, 3, 7):
        u, v = oracle.vort2vel(state["vor"][:, :, k], state["div"][:, :, k])
        ug, vg = oracle.spec2grid(u, 2), oracle.spec2grid(v, 2)
        ke_grid = ref.area_mean(0.5 * (ug * ug + vg * vg), wt)
        ke_spec = float((got["ke_rot_spectrum"][k] + got["ke_div_spectrum"][k]).sum())
        tg = oracle.spec2grid(state["t"][:, :, k], 1)
        t_mean = ref.area_mean(tg, wt)
        t_var = ref.area_mean((tg - t_mean) ** 2, wt)
        figures = (abs(ke_spec / ke_grid - 1.0), abs(float(got["t_spectrum"][k][1:].sum()) / t_var - 1.0),
                   abs(float(got["t_mean"][k]) / t_mean - 1.0))
        print("time level %d level %d: KE %.2e, T variance %.2e, T mean %.2e" % ((time_level, k) + figures))
        assert figures[0] < 2e-4 and figures[1] < 2e-3 and figures[2] < 2e-5, (k, figures)
        assert ke_grid > 1.0 and t_var > 1.0  # (a real state, not zeros)


def test_golden_tables_and_oracle_agree_on_elm2(oracle, golden_dir):
    """The arbiter may take elm2 from either: a^2 / (l (l + 1)) with the reference's radius, 0 at l = 0, a function of m + n."""
    golden = np.load(os.path.join(golden_dir, "tables.npz"))["elm2"]
    assert np.array_equal(golden, oracle.table("elm2"))
    per_l = ref.elm2_of_l(golden)
    assert per_l[0] == 0.0
    a = 6.371e6
    l = np.arange(1, 32)
    assert np.allclose(per_l[1:], a * a / (l * (l + 1.0)), rtol=1e-6, atol=0.0)
    for m in range(31):
        for n in range(32):
            if m + n <= 31:
                assert golden[m, n] == per_l[m + n]


def test_the_golden_states_vanish_beyond_the_truncation(run):
    """Every golden state has exactly zero coefficients at m + n > 31: what the bins leave out holds nothing."""
    m, n = np.meshgrid(np.arange(31), np.arange(32), indexing="ij")
    beyond = (m + n) > 31
    for day in ("d0", "d1", "d3"):
        for name in ("vor", "div", "t", "tr", "ps"):
            x = run["%s_%s" % (day, name)]
            assert not np.any(x[beyond]), (day, name)
            assert np.any(x[~beyond])


def test_arbiter_bins_a_single_coefficient():
    """One coefficient at (m, n) lands in bin m + n with weight 1 (m = 0) or 2, halved; the mean is Re f_0^0 sqrt(1/2)."""
    elm2 = np.ones((31, 32))
    zero3, zero2 = np.zeros((31, 32, 8), dtype=complex), np.zeros((31, 32), dtype=complex)
    for m, n, weight in ((0, 5, 1.0), (3, 4, 2.0), (30, 1, 2.0), (0, 31, 1.0)):
        t = zero3.copy()
        t[m, n, 2] = 3.0 - 4.0j
        got = ref.spectra(zero3, zero3, t, zero3, zero2, elm2)
        want = np.zeros((8, 32))
        want[2, m + n] = 0.5 * weight * 25.0
        assert np.array_equal(got["t_spectrum"], want), (m, n)
    t = zero3.copy()
    t[0, 0, :] = 2.0 + 1.0j
    t[5, 27, :] = 1.0  # m + n = 32: not read
    got = ref.spectra(t, zero3, t, zero3, zero2, elm2)
    assert np.array_equal(got["t_mean"], np.full(8, 2.0 * ref.ROOT_HALF))
    assert np.array_equal(got["t_spectrum"][:, 0], np.full(8, 2.5)) and not got["t_spectrum"][:, 1:].any()
    assert np.array_equal(got["ke_rot_spectrum"][:, 0], np.full(8, 0.25 * 5.0))


def test_spectra_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd._lib as L
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in SPECTRA_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name


def test_python_names_match_the_arbiter():
    from pyspeedy_amd.model import EnsembleModel
    assert EnsembleModel.SPECTRA_NAMES == ref.NAMES
    assert set(EnsembleModel.SPECTRA_DERIVED) == {"ke_spectrum", "ke_mean", "ke_column"}
    for method in ("spectra_configure", "spectra_reset", "spectra_info", "spectra_steps", "spectra_times", "spectra", "spectrum"):
        assert callable(getattr(EnsembleModel, method)), method


def _names(*names):
    return (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])


@pytest.mark.parametrize("names, every, capacity, message", [
    (("t_spectrum", "ke_spectrum"), 1, 4, b"unknown name 'ke_spectrum'"),
    (("t_spectrum", "t_grid"), 1, 4, b"unknown name 't_grid'"),
    (("t_mean", "t_mean"), 1, 4, b"given twice"),
    (("lnps_mean",), 0, 4, b"every must be at least 1"),
    (("lnps_mean",), -3, 4, b"every must be at least 1"),
    (("ke_rot_spectrum",), 1, 0, b"capacity must be at least 1"),
    (ref.NAMES, 1, 4, b"null model"),
])
def test_configure_checks_its_arguments_first(hip_lib, names, every, capacity, message):
    rc = hip_lib.spd_model_spectra_configure(None, _names(*names), len(names), every, capacity)
    assert rc == -1
    assert message in hip_lib.spd_last_error()
    assert b"spd_model_spectra_configure" in hip_lib.spd_last_error()


def test_argument_checks_come_in_the_documented_order(hip_lib):
    """unknown name, name twice, every, capacity, then the null model"""
    cases = [(("olr", "olr"), 0, 0, b"unknown name"), (("q_mean", "q_mean"), 0, 0, b"given twice"), (("q_mean",), 0, 0, b"every must"),
             (("q_mean",), 1, 0, b"capacity must"), (("q_mean",), 1, 1, b"null model")]
    for names, every, capacity, message in cases:
        assert hip_lib.spd_model_spectra_configure(None, _names(*names), len(names), every, capacity) == -1
        assert message in hip_lib.spd_last_error(), (message, hip_lib.spd_last_error())


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    buf = C.c_double()
    taken, held = C.c_longlong(), C.c_int()
    rows = (C.c_int32 * 6)()
    assert hip_lib.spd_model_spectra_configure(None, None, -1, 1, 4) == -1
    assert b"spd_model_spectra_configure" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_spectra_configure(None, None, 0, 1, 4) == -1  # (switching off still needs a model)
    assert b"spd_model_spectra_configure: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_spectra_reset(None) == -1 and b"spd_model_spectra_reset" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_spectra_info(None, C.byref(taken), C.byref(held), None, None) == -1
    assert b"spd_model_spectra_info" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_spectra_times(None, rows, 1) == -1 and b"spd_model_spectra_times" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_spectra_read(None, b"t_mean", 0, 1, 0, 1, C.byref(buf), 8, None) == -1
    assert b"spd_model_spectra_read" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_spectra_compute(None, _names("t_mean"), 1, 0, 1, C.byref(buf), 8, None) == -1
    assert b"spd_model_spectra_compute: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_spectra_compute(None, _names("t_mean", "olr"), 2, 0, 1, C.byref(buf), 8, None) == -1
    assert b"spd_model_spectra_compute: unknown name 'olr'" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_spectra_compute(None, _names("q_mean", "q_mean"), 2, 0, 1, C.byref(buf), 8, None) == -1
    assert b"given twice" in hip_lib.spd_last_error()


def test_energy_spectrum_example_parses_its_arguments_and_fits_a_slope():
    spec = importlib.util.spec_from_file_location("energy_spectrum", os.path.join(ROOT, "examples", "energy_spectrum.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.days, args.call_days, args.start, args.noise, args.level) == (64, 10, 1, "1982-01", 0.01, 2)
    args = mod.parse(["--members", "8", "--days", "3", "--call-days", "2", "--start", "1983-06", "--noise", "0.1", "--level", "7"])
    assert (args.members, args.days, args.call_days, args.start, args.noise, args.level) == (8, 3, 2, "1983-06", 0.1, 7)
    for bad in (["--members", "1"], ["--days", "0"], ["--level", "8"], ["--level", "-1"]):
        with pytest.raises(SystemExit):
            mod.parse(bad)
    l = np.arange(32, dtype=float)
    assert abs(mod.slope(np.where(l > 0, np.maximum(l, 1.0) ** -3.0, 1.0)) + 3.0) < 1e-12
