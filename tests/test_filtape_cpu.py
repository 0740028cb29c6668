"""CPU tier: the filter tape's entry points (spd_model_filtape_*, spd_filtape_check, spd_filtape_filter_host) are declared, exported
and bound; the argument checks the library makes before it needs a model or a device, in their documented order; the filter step --
spd_filtape_filter_host, the host compile of the routines the kernel runs (csrc/filter_point.hpp) -- bitwise against the numpy
restatement (tests/filtape_reference.py), and that against a loop over Python floats; pyspeedy_amd.butterworth_sections against the
analytic Butterworth magnitude and, where it is installed, against scipy.signal; the storm-track example parses its arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import filtape_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTAPE_SYMBOLS = ("spd_model_filtape_configure", "spd_model_filtape_off", "spd_model_filtape_reset", "spd_model_filtape_info",
                   "spd_model_filtape_times", "spd_model_filtape_read", "spd_filtape_check", "spd_filtape_filter_host")
DP = C.POINTER(C.c_double)


def test_filtape_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd
    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in FILTAPE_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for method in ("filtape_configure", "filtape_off", "filtape_reset", "filtape_info", "filtape_entries", "filtape_steps", "filtape_times",
                   "filtape_counts", "filtape"):
        assert hasattr(EnsembleModel, method), method
    assert isinstance(EnsembleModel.filtape_info, property) and isinstance(EnsembleModel.filtape_entries, property)
    assert callable(pyspeedy_amd.butterworth_sections) and "butterworth_sections" in pyspeedy_amd.__all__
    # the constants agree: header, Fortran, _lib, the reference and the Python names
    assert "#define SPD_FIL_MEAN 0\n" in header and "#define SPD_FIL_COV 1\n" in header and "#define SPD_FIL_LAST 2\n" in header
    assert "SPD_FIL_MEAN = 0, SPD_FIL_COV = 1, SPD_FIL_LAST = 2" in fortran
    assert (L.SPD_FIL_MEAN, L.SPD_FIL_COV, L.SPD_FIL_LAST) == (0, 1, 2) == (ref.MEAN, ref.COV, ref.LAST)
    assert EnsembleModel.FILTAPE_OPS == {"mean": 0, "cov": 1, "last": 2}


# ---- the filter step: the library's host compile, the numpy restatement and the loop over Python floats -------------------------------
def host_filter(hip_lib, sections, x):
    sections = np.ascontiguousarray(sections, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.full_like(x, -1.0)
    rc = hip_lib.spd_filtape_filter_host(sections.ctypes.data_as(DP), sections.shape[0], x.ctypes.data_as(DP), x.size, y.ctypes.data_as(DP))
    assert rc == 0, hip_lib.spd_last_error()
    return y


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def cascades():
    """(label, sections): one, two and four sections; band-pass, low-pass and high-pass"""
    import pyspeedy_amd
    bw = pyspeedy_amd.butterworth_sections
    return [("lowpass 1 section", bw("lowpass", 2, 10.0, 1.0)), ("lowpass 2 sections", bw("lowpass", 3, 40.0, 1.0)),
            ("lowpass 4 sections", bw("lowpass", 8, 12.0, 1.0)), ("highpass 1 section", bw("highpass", 1, 6.0, 1.0)),
            ("highpass 2 sections", bw("highpass", 4, 8.0, 1.0)), ("highpass 4 sections", bw("highpass", 7, 5.0, 1.0)),
            ("bandpass 1 section", bw("bandpass", 1, (8.0, 24.0), 1.0)), ("bandpass 2 sections", bw("bandpass", 2, (8.0, 24.0), 1.0)),
            ("bandpass 4 sections", bw("bandpass", 4, (2.5, 30.0), 1.0))]


def test_host_filter_equals_the_arbiter_bitwise(hip_lib):
    """Seeded series of 40 samples with a large mean, 5500 + N(0, 50), through cascades of 1, 2 and 4 sections of all three kinds: the
    library's host compile, the numpy restatement (over a [40][3] array and over a scalar series) and the loop over Python floats
    give the same bits, and the filters do something: the output is not the input and not constant."""
    shapes = {"1 section": 1, "2 sections": 2, "4 sections": 4}
    for seed, (label, sections) in enumerate(cascades()):
        assert sections.shape == (shapes[label.split(" ", 1)[1]], 5), label
        x = 5500.0 + np.random.default_rng(seed).normal(0.0, 50.0, (40, 3))
        by_numpy = ref.filter_series(sections, x)
        for col in range(3):
            got = host_filter(hip_lib, sections, x[:, col])
            by_floats = np.array(ref.filter_scalar(sections, x[:, col].tolist()))
            assert np.array_equal(bits(got), bits(by_floats)), (label, col, np.abs(got - by_floats).max())
            assert np.array_equal(bits(by_numpy[:, col]), bits(by_floats)), (label, col)
            assert np.ptp(got) > 1.0 and np.abs(got - x[:, col]).max() > 1.0, label
        if label.startswith("bandpass") or label.startswith("highpass"):  # no ringing from the large mean: the output stays near zero
            assert np.abs(by_numpy).max() < 200.0, (label, np.abs(by_numpy).max())


def test_a_constant_series_is_in_steady_state_from_the_first_sample(hip_lib):
    """The first sample of a constant x gives g x section after section, exactly; a band-pass gives exactly 0.0 at every sample; the
    later samples of the other kinds stay at that value to rounding (the steady state is a fixed point of the exact recursion; what
    rounding adds per sample is a few ulp of the terms, which the poles damp: 1e-12 relative is orders above it and far below the
    O(1) ringing of a filter started from rest)."""
    x = np.full(40, 5500.0)
    for label, sections in cascades():
        got = host_filter(hip_lib, sections, x)
        first = 5500.0
        for s in sections:
            first = ref.gain(s) * first
        assert got[0] == first, (label, got[0], first)
        if label.startswith("bandpass"):
            assert np.array_equal(bits(got), bits(np.zeros(40))), (label, got)  # +0.0, bit for bit
        else:
            expected = 5500.0 if label.startswith("lowpass") else 0.0
            assert abs(first - expected) <= 1e-9, (label, first)
            assert np.abs(got - first).max() <= 1e-12 * 5500.0, (label, np.abs(got - first).max())
    from_rest = ref.filter_series(cascades()[0][1], np.concatenate([[0.0], x]))  # (what the steady start avoids)
    assert np.abs(from_rest[1:6] - 5500.0).max() > 100.0


def test_filter_host_refuses_bad_arguments(hip_lib):
    ok = np.array([[0.2, 0.4, 0.2, -0.5, 0.3]])
    x = np.zeros(4)
    y = np.zeros(4)

    def call(sections, n_sections, xs=x, n=4):
        s = None if sections is None else np.ascontiguousarray(sections, dtype=np.float64).ctypes.data_as(DP)
        return hip_lib.spd_filtape_filter_host(s, n_sections, None if xs is None else xs.ctypes.data_as(DP), n, y.ctypes.data_as(DP))

    bad = ok.copy()
    bad[0, 1] = np.inf
    unstable = ok.copy()
    unstable[0, 4] = 1.0
    for args, message in (((ok, 0), b"n_sections must be 1 ... 4, got 0"), ((ok, 5), b"n_sections must be 1 ... 4, got 5"),
                          ((None, 1), b"null sections"), ((bad, 1), b"section 0 holds a coefficient that is not finite"),
                          ((unstable, 1), b"section 0 is not stable"), ((ok, 1, x, -1), b"bad series"), ((ok, 1, None, 4), b"bad series")):
        assert call(*args) == -1
        assert message in hip_lib.spd_last_error() and b"spd_filtape_filter_host" in hip_lib.spd_last_error(), hip_lib.spd_last_error()
    assert call(ok, 1, x, 0) == 0


# ---- butterworth_sections ---------------------------------------------------------------------------------------------------------
DESIGNS = [(kind, order, periods) for kind, orders, edges in (("lowpass", range(1, 9), (3.0, 10.0, 40.0)), ("highpass", range(1, 9), (3.0, 10.0, 40.0)),
                                                                ("bandpass", range(1, 5), ((8.0, 24.0), (2.5, 60.0), (5.0, 6.0))))
           for order in orders for periods in edges]
# The bound on | |H|^2 - 1 / (1 + W^2N) |.  A section's response is a ratio of two sums of three terms of size O(1), evaluated in
# fp64 from coefficients that are themselves rounded: its relative error is a few eps divided by the distance of e^{i omega} to the
# nearest pole, which for the designs below (the 40-sample low-pass of order 8 has poles at radius 0.99) is no smaller than 0.01;
# with at most four sections and |H|^2 <= 1 that gives about 4 * 4 * 2.2e-16 / 0.01 = 4e-13.  Observed maximum over DESIGNS: 2.0e-14
# (DESIGN section 4q); the bound is 1e-12, within 100 times what was observed and far inside the 1e-9 the recorder's users need.
RESPONSE_BOUND = 1e-12


def response_error(kind, order, periods):
    import pyspeedy_amd
    sections = pyspeedy_amd.butterworth_sections(kind, order, periods, 1.0)
    assert sections.shape == (order if kind == "bandpass" else (order + 1) // 2, 5) and sections.dtype == np.float64
    for s in sections:
        assert ref.stable(s), (kind, order, periods, s)
    _, special = ref.butterworth_magnitude2(kind, order, periods, 1.0, np.array([1.0]))
    omega = np.concatenate([special, np.linspace(0.01, np.pi - 0.01, 64)])
    analytic, _ = ref.butterworth_magnitude2(kind, order, periods, 1.0, omega)
    got = ref.magnitude2(sections, omega)
    n_edges = 2 if kind == "bandpass" else 1
    assert np.abs(analytic[:n_edges] - 0.5).max() < 1e-12  # (the arbiter's own edges: one half)
    if kind == "bandpass":
        assert abs(analytic[2] - 1.0) < 1e-15  # (and its centre: one)
    return sections, omega, got, float(np.abs(got - analytic).max())


def test_butterworth_sections_have_the_butterworth_magnitude():
    worst = 0.0
    for kind, order, periods in DESIGNS:
        _, _, _, err = response_error(kind, order, periods)
        worst = max(worst, err)
        assert err <= RESPONSE_BOUND, (kind, order, periods, err)
    print("butterworth_sections: max | |H|^2 - analytic | over %d designs and 65 to 67 frequencies each: %.3e" % (len(DESIGNS), worst))


def test_butterworth_sections_agree_with_scipy():
    signal = pytest.importorskip("scipy.signal")
    for kind, order, periods in DESIGNS:
        _, omega, got, _ = response_error(kind, order, periods)
        edges = np.sort(2.0 / np.atleast_1d(np.asarray(periods, dtype=np.float64)))  # in units of the Nyquist frequency
        sos = signal.butter(order, edges if kind == "bandpass" else edges[0], kind, output="sos")
        _, h = signal.sosfreqz(sos, worN=omega)
        assert np.abs(np.abs(h) ** 2 - got).max() <= 2.0 * RESPONSE_BOUND, (kind, order, periods)  # (each within the bound of the analytic one)


def test_butterworth_sections_units_and_refusals():
    import pyspeedy_amd
    bw = pyspeedy_amd.butterworth_sections
    # periods and the sampling interval in one unit: 2-6 days from six-hourly samples is 8-24 samples
    assert np.array_equal(bw("bandpass", 2, (2.0, 6.0), 0.25), bw("bandpass", 2, (24.0, 8.0), 1.0))
    assert np.array_equal(bw("lowpass", 3, 240.0, 6.0), bw("lowpass", 3, 40.0, 1.0))
    for args, message in ((("notch", 2, 10.0, 1.0), "kind must be"), (("lowpass", 0, 10.0, 1.0), "order must be 1 ... 8"),
                          (("bandpass", 5, (8.0, 24.0), 1.0), "order must be 1 ... 4"), (("lowpass", 2, (8.0, 24.0), 1.0), "one period"),
                          (("bandpass", 2, 8.0, 1.0), "two periods"), (("lowpass", 2, 2.0, 1.0), "longer than two sample intervals"),
                          (("highpass", 2, 10.0, 0.0), "longer than two sample intervals"), (("bandpass", 2, (8.0, 8.0), 1.0), "must differ")):
        with pytest.raises(ValueError, match=message):
            bw(*args)


# ---- the argument checks that need neither a model nor a device ---------------------------------------------------------------------
LOW = [[0.2, 0.4, 0.2, -0.5, 0.3]]
BAND = [[0.2, 0.0, -0.2, -1.0, 0.6], [0.3, 0.0, -0.3, -0.4, 0.5]]
STEPS, DAY, MONTH = 0, 1, 2
GOOD = dict(filters=(LOW, BAND), rows=(("z_plev", 2, 1, 1), ("v_plev", 1, 1, 1, "t_plev", 1), ("mslp", 0, 1, 2), ("precnv", 0, 0, 0)),
            window=STEPS, every=12, sample_every=3, spinup=5, capacity=4, dtype=0)
FOURTEEN = b"(u_grid, v_grid, t_grid, q_grid, phi_grid, ps_grid, precnv, precls, u_plev, v_plev, t_plev, q_plev, z_plev, mslp)"


def _call(hip_lib, symbol, filters, rows, window, every, sample_every, spinup, capacity, dtype, n_filters=None, n_entries=None, arrays=True,
          sections=True):
    flat = np.ascontiguousarray([s for f in filters for s in f], dtype=np.float64).reshape(-1, 5)
    counts = (C.c_int * max(len(filters), 1))(*[len(f) for f in filters])
    n = max(len(rows), 1)
    names_a = (C.c_char_p * n)(*[r[0].encode() for r in rows])
    names_b = (C.c_char_p * n)(*[(r[4].encode() if len(r) == 6 else None) for r in rows])
    cols = [(C.c_int * n)(*[(r[k] if len(r) > k else 0) for r in rows]) for k in (1, 2, 3, 5)]
    args = [flat.ctypes.data_as(DP) if sections else None, counts if sections else None, len(filters) if n_filters is None else n_filters]
    args += [names_a, cols[0], cols[1], cols[2], names_b, cols[3]] if arrays else [None] * 6
    args += [len(rows) if n_entries is None else n_entries, window, every, sample_every, spinup, capacity, dtype]
    fn = getattr(hip_lib, symbol)
    return fn(None, *args) if symbol == "spd_model_filtape_configure" else fn(*args)


def with_(**changes):
    return dict(GOOD, **changes)


NAN_LOW = [[0.2, float("nan"), 0.2, -0.5, 0.3]]
FORTY_PLANES = tuple(("t_grid", level, f, 0) for f in range(5) for level in range(8))  # 40 distinct planes in 40 entries


@pytest.mark.parametrize("kw, message", [
    (with_(filters=()), b"n_filters must be 1 ... 8, got 0"),
    (with_(filters=(LOW,) * 9), b"n_filters must be 1 ... 8, got 9"),
    (with_(sections=False), b"null filters"),
    (with_(filters=(LOW, LOW * 5)), b"filter 1 must have 1 ... 4 sections, got 5"),
    (with_(filters=(LOW, [])), b"filter 1 must have 1 ... 4 sections, got 0"),
    (with_(filters=(LOW, [BAND[0], [0.1, 0.0, float("inf"), 0.0, 0.0]])), b"filter 1, section 1 holds a coefficient that is not finite"),
    (with_(filters=(NAN_LOW, BAND)), b"filter 0, section 0 holds a coefficient that is not finite"),
    (with_(filters=(LOW, [BAND[0], [1.0, 0.0, 0.0, 0.0, 1.0]])), b"filter 1, section 1 is not stable"),
    (with_(filters=([[1.0, 0.0, 0.0, 1.5, 0.5]], BAND)), b"filter 0, section 0 is not stable"),
    (with_(filters=([[1.0, 0.0, 0.0, -1.6, 0.5]], BAND)), b"filter 0, section 0 is not stable"),
    (with_(filters=([[1.0, 0.0, 0.0, 0.0, -1.0]], BAND)), b"filter 0, section 0 is not stable"),
    (with_(rows=()), b"n_entries must be 1 ... 64, got 0"),
    (with_(rows=(("t_grid", 0, 0, 0),) * 65), b"n_entries must be 1 ... 64, got 65"),
    (with_(arrays=False), b"bad list of entries"),
    (with_(rows=(("z_plev", 2, 1, 1), ("olr", 0, 0, 0))), b"unknown variable 'olr' " + FOURTEEN),
    (with_(rows=(("v_plev", 1, 1, 1, "wspd_grid", 1),)), b"unknown variable 'wspd_grid' " + FOURTEEN),
    (with_(rows=(("t_grid", 8, 0, 0),)), b"level 8 of entry 0 ('t_grid') is out of range (0 ... 7)"),
    (with_(rows=(("z_plev", 2, 1, 1), ("mslp", 1, 0, 0))), b"level 1 of entry 1 ('mslp') is out of range (0 ... 0)"),
    (with_(rows=(("z_plev", -1, 1, 1),)), b"level -1 of entry 0 ('z_plev') is out of range"),
    (with_(rows=(("u_grid", 2, 0, 1, "precnv", 1),)), b"level 1 of entry 0 ('precnv') is out of range (0 ... 0)"),
    (with_(rows=(("t_grid", 0, 2, 0),)), b"filter 2 of entry 0 ('t_grid') is out of range (0 ... 1)"),
    (with_(rows=(("z_plev", 2, 1, 1), ("t_grid", 0, -1, 0))), b"filter -1 of entry 1 ('t_grid') is out of range (0 ... 1)"),
    (with_(rows=(("t_grid", 0, 1, 3),)), b"op 3 of entry 0 ('t_grid') is not SPD_FIL_MEAN (0), SPD_FIL_COV (1) or SPD_FIL_LAST (2)"),
    (with_(rows=(("t_grid", 0, 1, -1),)), b"op -1 of entry 0 ('t_grid') is not SPD_FIL_MEAN"),
    (with_(rows=(("v_plev", 1, 1, 0, "t_plev", 1),)), b"entry 0 ('v_plev') names a second field ('t_plev'), which only SPD_FIL_COV takes"),
    (with_(rows=(("z_plev", 2, 1, 1), ("v_plev", 1, 1, 2, "t_plev", 1))), b"entry 1 ('v_plev') names a second field ('t_plev')"),
    (with_(filters=(LOW,) * 5, rows=FORTY_PLANES), b"the entries name 40 distinct (name, level, filter) planes; at most 32"),
    (with_(spinup=-1), b"spinup must not be negative"),
    (with_(window=3), b"unknown window kind 3"),
    (with_(every=0), b"every must be at least 1 for SPD_WINDOW_STEPS"),
    (with_(window=DAY), b"every must be 0 for SPD_WINDOW_DAY and SPD_WINDOW_MONTH"),
    (with_(window=MONTH), b"every must be 0 for SPD_WINDOW_DAY and SPD_WINDOW_MONTH"),
    (with_(sample_every=0), b"sample_every must be at least 1"),
    (with_(capacity=0), b"capacity must be at least 1"),
    (with_(dtype=2), b"dtype must be SPD_TAPE_F32 or SPD_TAPE_F64"),
])
def test_the_checks_refuse_with_a_message(hip_lib, kw, message):
    for symbol in ("spd_filtape_check", "spd_model_filtape_configure"):
        assert _call(hip_lib, symbol, **kw) == -1, (symbol, message)
        assert message in hip_lib.spd_last_error(), hip_lib.spd_last_error()
        assert symbol.encode() in hip_lib.spd_last_error()


def test_what_the_checks_accept(hip_lib):
    """A configuration that is fine until a model is needed: spd_filtape_check says so, _configure reaches the null model.  The same
    plane under two filters, the same entry twice, 32 distinct planes in 64 entries, a derived and a pressure-level name whose level
    only a model can judge, both calendar windows."""
    thirty_two = tuple(("t_grid", level, f, 1, "u_grid", level) for f in range(2) for level in range(8))  # 2 x 8 x 2 planes
    for kw in (GOOD, with_(window=DAY, every=0), with_(window=MONTH, every=0, spinup=0, dtype=1),
               with_(rows=(("z_plev", 31, 0, 0), ("tcwv", 0, 1, 2), ("z_plev", 31, 1, 0), ("z_plev", 31, 1, 0), ("omega_plev", 7, 1, 1))),
               with_(rows=thirty_two * 2), with_(filters=(LOW * 4,) * 8, rows=(("t_grid", 0, 7, 0),))):
        assert _call(hip_lib, "spd_filtape_check", **kw) == 0, hip_lib.spd_last_error()
        assert _call(hip_lib, "spd_model_filtape_configure", **kw) == -1
        assert b"spd_model_filtape_configure: null model" in hip_lib.spd_last_error(), hip_lib.spd_last_error()


def test_argument_checks_come_in_the_documented_order(hip_lib):
    """n_filters, null filters, the number of sections, a coefficient that is not finite, an unstable section, n_entries, null lists,
    an unknown name (a's, then b's), per entry level_a, level_b, filter, op and a second field where none is taken, the number of
    filtered planes, spinup, window kind, every, sample_every, capacity, dtype, then the null model: each case is wrong in everything
    that comes later as well."""
    bad_sections = ([[float("nan"), 0.0, 0.0, 0.0, 2.0]] * 5, LOW)   # five sections, not finite AND unstable
    nan_unstable = ([[float("nan"), 0.0, 0.0, 0.0, 2.0]], LOW)
    unstable = ([[1.0, 0.0, 0.0, 0.0, 2.0]], LOW)
    good = (LOW,) * 5
    tail = dict(window=9, every=-1, sample_every=0, spinup=-1, capacity=0, dtype=9)
    bad_row = ("olr", 9, 9, 9, "wspd_plev", 9)
    many = tuple(("t_grid", level, f, 0) for f in range(5) for level in range(8))
    cases = [(dict(filters=bad_sections, rows=(bad_row,), n_filters=0, n_entries=99, arrays=False, sections=False, **tail), b"n_filters must"),
             (dict(filters=bad_sections, rows=(bad_row,), n_entries=99, arrays=False, sections=False, **tail), b"null filters"),
             (dict(filters=bad_sections, rows=(bad_row,), n_entries=99, arrays=False, **tail), b"filter 0 must have 1 ... 4 sections, got 5"),
             (dict(filters=nan_unstable, rows=(bad_row,), n_entries=99, arrays=False, **tail), b"is not finite"),
             (dict(filters=unstable, rows=(bad_row,), n_entries=99, arrays=False, **tail), b"is not stable"),
             (dict(filters=good, rows=(bad_row,), n_entries=99, arrays=False, **tail), b"n_entries must be 1 ... 64, got 99"),
             (dict(filters=good, rows=(bad_row,), arrays=False, **tail), b"bad list of entries"),
             (dict(filters=good, rows=(bad_row,), **tail), b"unknown variable 'olr'"),
             (dict(filters=good, rows=(("t_grid",) + bad_row[1:],), **tail), b"unknown variable 'wspd_plev'"),
             (dict(filters=good, rows=(("t_grid", 9, 9, 9, "mslp", 9),), **tail), b"level 9 of entry 0 ('t_grid')"),
             (dict(filters=good, rows=(("t_grid", 0, 9, 9, "mslp", 9),), **tail), b"level 9 of entry 0 ('mslp')"),
             (dict(filters=good, rows=(("t_grid", 0, 9, 9, "mslp", 0),), **tail), b"filter 9 of entry 0"),
             (dict(filters=good, rows=(("t_grid", 0, 0, 9, "mslp", 0),), **tail), b"op 9 of entry 0"),
             (dict(filters=good, rows=(("t_grid", 0, 0, 2, "mslp", 0),) + many, **tail), b"names a second field"),
             (dict(filters=good, rows=many, **tail), b"40 distinct"),
             (dict(filters=good, rows=many[:8], **tail), b"spinup must not be negative"),
             (dict(filters=good, rows=many[:8], **dict(tail, spinup=0)), b"unknown window kind 9"),
             (dict(filters=good, rows=many[:8], **dict(tail, spinup=0, window=STEPS)), b"every must be at least 1"),
             (dict(filters=good, rows=many[:8], **dict(tail, spinup=0, window=STEPS, every=1)), b"sample_every must be at least 1"),
             (dict(filters=good, rows=many[:8], **dict(tail, spinup=0, window=STEPS, every=1, sample_every=1)), b"capacity must be at least 1"),
             (dict(filters=good, rows=many[:8], **dict(tail, spinup=0, window=STEPS, every=1, sample_every=1, capacity=1)), b"dtype must be"),
             (dict(filters=good, rows=many[:8], window=STEPS, every=1, sample_every=1, spinup=0, capacity=1, dtype=1), b"null model")]
    for kw, message in cases:
        assert _call(hip_lib, "spd_model_filtape_configure", **kw) == -1
        assert message in hip_lib.spd_last_error(), (message, hip_lib.spd_last_error())


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    buf = C.c_double()
    rows = (C.c_int32 * 8)()
    for symbol, args in (("spd_model_filtape_off", ()), ("spd_model_filtape_reset", ()), ("spd_model_filtape_info", (None,) * 12),
                         ("spd_model_filtape_times", (rows, 1)), ("spd_model_filtape_read", (0, 0, 1, 0, 1, C.byref(buf), 8, None))):
        assert getattr(hip_lib, symbol)(None, *args) == -1, symbol
        assert b"null model" in hip_lib.spd_last_error() and symbol.encode() in hip_lib.spd_last_error(), hip_lib.spd_last_error()


# ---- the arbiter's own bookkeeping, and the example --------------------------------------------------------------------------------
def test_the_arbiter_counts_samples_as_the_definition_says():
    """Windows of 12 steps, a sample every 3, spin-up 5 over 48 steps: filter samples 1 ... 5 (steps 3 ... 15) are counted nowhere, so
    the first window is empty and the second holds steps 18, 21, 24; and the reduction of a known series."""
    steps = list(range(3, 49, 3))
    rows = [[12], [24], [36], [48]]
    assert ref.counted_windows(rows, 0, steps, 5) == [[], [5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]]
    assert ref.counted_windows(rows, 0, steps, 0) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]]
    assert ref.counted_windows(rows[2:], 24, steps[8:], 2, first_k=1) == [[2, 3], [4, 5, 6, 7]]
    ya = np.arange(16.0).reshape(16, 1) + 1.0
    yb = 2.0 * ya
    windows = [[], [5, 6, 7], [8]]
    assert np.array_equal(ref.reduce_windows(ya, yb, ref.MEAN, windows)[1:], [[7.0], [9.0]])
    assert np.array_equal(ref.reduce_windows(ya, yb, ref.COV, windows)[1:], [[(72.0 + 98.0 + 128.0) / 3.0], [162.0]])
    assert np.array_equal(ref.reduce_windows(ya, yb, ref.LAST, windows)[1:], [[8.0], [9.0]])
    for op in (ref.MEAN, ref.COV, ref.LAST):
        assert np.isnan(ref.reduce_windows(ya, yb, op, windows)[0]).all()


def test_example_parses_its_arguments():
    path = os.path.join(ROOT, "examples", "bandpass_storm_tracks.py")
    spec = importlib.util.spec_from_file_location("bandpass_storm_tracks", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    args = module.parse_args(["--members", "4", "--months", "2"])
    assert args.members == 4 and args.months == 2
    filters = module.filters()
    assert [f.shape for f in filters] == [(2, 5), (1, 5)]
    for f in filters:
        for s in f:
            assert ref.stable(s)
    assert len(module.entries()) == 5
