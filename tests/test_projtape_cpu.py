"""CPU tier: the projection tape's entry points (spd_model_projtape_*) are declared, exported and bound; the numpy restatement of its
sum (tests/projtape_reference.py) against a loop over Python floats; the argument checks the library makes before it needs a model or
a device, in their documented order; pyspeedy_amd.projection_weights; the climate-indices example parses its arguments."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

import projtape_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJTAPE_SYMBOLS = ("spd_model_projtape_configure", "spd_model_projtape_reset", "spd_model_projtape_info", "spd_model_projtape_times",
                    "spd_model_projtape_read")
FOURTEEN = b"(u_grid, v_grid, t_grid, q_grid, phi_grid, ps_grid, precnv, precls, u_plev, v_plev, t_plev, q_plev, z_plev, mslp)"
SEED = 0  # (chosen here so that np.sum differs from the stated order in at least one of the planes below)


def test_projtape_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd
    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in PROJTAPE_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for method in ("projtape_configure", "projtape_reset", "projtape_info", "projtape_steps", "projtape_times", "projtape",
                   "projtape_entries"):
        assert hasattr(EnsembleModel, method), method
    assert isinstance(EnsembleModel.projtape_info, property) and isinstance(EnsembleModel.projtape_entries, property)
    assert pyspeedy_amd.projection_weights is L.projection_weights and "projection_weights" in pyspeedy_amd.__all__


def test_the_numpy_restatement_is_the_stated_order_and_not_np_sum():
    """project() is bitwise the loop over Python floats on seeded random planes with weights of both signs, also through its batch
    dimensions; np.sum(w * x) differs from it in at least one of them -- otherwise "bitwise" would pin nothing."""
    rng = np.random.default_rng(SEED)
    differs = 0
    for case in range(6):
        w = rng.normal(0.0, 1.0, (48, 96))
        x = 250.0 + 30.0 * rng.normal(0.0, 1.0, (48, 96))
        assert (w < 0).any() and (w > 0).any()
        got, loop = ref.project(w, x), ref.project_loop(w, x)
        assert got.shape == () and got.dtype == np.float64
        assert float(got).hex() == loop.hex(), case
        assert abs(float(got) - float(np.sum(w * x))) <= 1e-9 * np.sum(np.abs(w * x))  # (the same sum, to rounding)
        differs += float(np.sum(w * x)).hex() != loop.hex()
    assert differs >= 1
    w = rng.normal(0.0, 1.0, (48, 96))
    x = rng.normal(0.0, 1.0, (2, 3, 48, 96))
    batch = ref.project(w, x)
    assert batch.shape == (2, 3)
    assert ref.project(w.reshape(-1), x.reshape(2, 3, 4608)).tolist() == batch.tolist()
    for a in range(2):
        for b in range(3):
            assert float(batch[a, b]).hex() == ref.project_loop(w, x[a, b]).hex()
    # a term of zero weight takes part: -0.0 + 0.0 * x is not skipped, and an infinite x under a zero weight gives NaN
    w0 = np.zeros((48, 96))
    assert float(ref.project(w0, np.full((48, 96), 3.0))) == 0.0
    x_inf = np.full((48, 96), 1.0)
    x_inf[5, 7] = np.inf
    with np.errstate(invalid="ignore"):
        assert math.isnan(float(ref.project(w0, x_inf))) and math.isnan(ref.project_loop(w0, x_inf))


# ---- the argument checks that need neither a model nor a device --------------------------------------------------------
def _call(hip_lib, weights, n_patterns, triples, every, capacity, n_entries=None, arrays=True):
    n = max(len(triples), 1)
    names = (C.c_char_p * n)(*[t[0].encode() for t in triples])
    levels = (C.c_int * n)(*[t[1] for t in triples])
    patterns = (C.c_int * n)(*[t[2] for t in triples])
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    if not arrays:
        names = levels = patterns = None
    return hip_lib.spd_model_projtape_configure(None, w, n_patterns, names, levels, patterns, len(triples) if n_entries is None else n_entries,
                                                every, capacity)


ONES = np.ones((2, 48, 96))
NAN_AT = ONES.copy()
NAN_AT[1, 3, 5] = np.nan  # pattern 1, point 96 * 3 + 5 = 293
INF_AT = ONES.copy()
INF_AT[0, 47, 95] = -np.inf


@pytest.mark.parametrize("weights, n_patterns, triples, every, capacity, message", [
    (ONES, 2, (("t_grid", 7, 0),), 0, 4, b"every must be at least 1"),
    (ONES, 2, (("t_grid", 7, 0),), 3, 0, b"capacity must be at least 1"),
    (ONES, 0, (("t_grid", 7, 0),), 3, 4, b"n_patterns must be 1 ... 64, got 0"),
    (ONES, 65, (("t_grid", 7, 0),), 3, 4, b"n_patterns must be 1 ... 64, got 65"),
    (None, 2, (("t_grid", 7, 0),), 3, 4, b"null weights"),
    (NAN_AT, 2, (("t_grid", 7, 0),), 3, 4, b"weight of pattern 1 at point 293 (row 3, column 5) is not finite"),
    (INF_AT, 2, (("t_grid", 7, 0),), 3, 4, b"weight of pattern 0 at point 4607 (row 47, column 95) is not finite"),
    (ONES, 2, (("t_grid", 7, 0), ("olr", 0, 0)), 3, 4, b"unknown variable 'olr' " + FOURTEEN),
    (ONES, 2, (("wspd_grid", 0, 0),), 3, 4, b"unknown variable 'wspd_grid' " + FOURTEEN),
    (ONES, 2, (("t_grid", 8, 0),), 3, 4, b"level 8 of entry 0 ('t_grid') is out of range (0 ... 7)"),
    (ONES, 2, (("t_grid", 0, 0), ("mslp", 1, 0)), 3, 4, b"level 1 of entry 1 ('mslp') is out of range (0 ... 0)"),
    (ONES, 2, (("precnv", -1, 0),), 3, 4, b"level -1 of entry 0 ('precnv') is out of range (0 ... 0)"),
    (ONES, 2, (("z_plev", -1, 0),), 3, 4, b"level -1 of entry 0 ('z_plev') is out of range"),
    (ONES, 2, (("t_grid", 0, 2),), 3, 4, b"pattern 2 of entry 0 ('t_grid') is out of range (0 ... 1)"),
    (ONES, 2, (("t_grid", 0, 1), ("ps_grid", 0, -1)), 3, 4, b"pattern -1 of entry 1 ('ps_grid') is out of range (0 ... 1)"),
    # (the same plane under two patterns, the same entry twice and a pressure-level name are fine until a model is needed)
    (ONES, 2, (("t_grid", 7, 0), ("t_grid", 7, 1), ("t_grid", 7, 1), ("z_plev", 11, 0)), 3, 4, b"null model"),
])
def test_configure_checks_its_arguments_first(hip_lib, weights, n_patterns, triples, every, capacity, message):
    assert _call(hip_lib, weights, n_patterns, triples, every, capacity) == -1
    assert message in hip_lib.spd_last_error(), hip_lib.spd_last_error()
    assert b"spd_model_projtape_configure" in hip_lib.spd_last_error()


def test_argument_checks_come_in_the_documented_order(hip_lib):
    """every, capacity, n_patterns, n_entries, null weights, null lists, a weight that is not finite, an unknown name, per entry its
    level and then its pattern, then the null model: each case is wrong in everything that comes later as well."""
    bad = (("olr", 9, 9), ("t_grid", 9, 9))
    cases = [(dict(weights=None, n_patterns=0, triples=bad, every=0, capacity=0, n_entries=2000, arrays=False), b"every must"),
             (dict(weights=None, n_patterns=0, triples=bad, every=1, capacity=0, n_entries=2000, arrays=False), b"capacity must"),
             (dict(weights=None, n_patterns=0, triples=bad, every=1, capacity=1, n_entries=2000, arrays=False), b"n_patterns must"),
             (dict(weights=None, n_patterns=2, triples=bad, every=1, capacity=1, n_entries=2000, arrays=False), b"n_entries must be 0 ... 1024, got 2000"),
             (dict(weights=None, n_patterns=2, triples=bad, every=1, capacity=1, n_entries=-1, arrays=False), b"n_entries must be 0 ... 1024, got -1"),
             (dict(weights=None, n_patterns=2, triples=bad, every=1, capacity=1, arrays=False), b"null weights"),
             (dict(weights=NAN_AT, n_patterns=2, triples=bad, every=1, capacity=1, arrays=False), b"bad list of entries"),
             (dict(weights=NAN_AT, n_patterns=2, triples=bad, every=1, capacity=1), b"is not finite"),
             (dict(weights=ONES, n_patterns=2, triples=bad, every=1, capacity=1), b"unknown variable 'olr'"),
             (dict(weights=ONES, n_patterns=2, triples=bad[1:], every=1, capacity=1), b"level 9 of entry 0"),
             (dict(weights=ONES, n_patterns=2, triples=(("t_grid", 0, 9), ("t_grid", 9, 0)), every=1, capacity=1), b"pattern 9 of entry 0"),
             (dict(weights=ONES, n_patterns=2, triples=(("t_grid", 0, 1),), every=1, capacity=1), b"null model")]
    for kw, message in cases:
        assert _call(hip_lib, **kw) == -1
        assert message in hip_lib.spd_last_error(), (message, hip_lib.spd_last_error())


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    buf = C.c_double()
    taken, held = C.c_longlong(), C.c_int()
    rows = (C.c_int32 * 6)()
    # switching off looks at nothing but the model
    assert hip_lib.spd_model_projtape_configure(None, None, 0, None, None, None, 0, 0, 0) == -1
    assert b"spd_model_projtape_configure: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_projtape_reset(None) == -1 and b"spd_model_projtape_reset: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_projtape_info(None, C.byref(taken), C.byref(held), None, None, None, None) == -1
    assert b"spd_model_projtape_info: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_projtape_times(None, rows, 1) == -1 and b"spd_model_projtape_times: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_projtape_read(None, 0, 1, 0, 1, C.byref(buf), 8, None) == -1
    assert b"spd_model_projtape_read: null model" in hip_lib.spd_last_error()


# ---- projection_weights ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pw(hip_lib):
    import pyspeedy_amd
    return pyspeedy_amd.projection_weights()


def ulps_from_one(w):
    return abs(math.fsum(w.ravel()) - 1.0) / np.finfo(np.float64).eps


def test_the_grid_is_the_export_s(pw, hip_lib):
    """48 Gaussian rows from south to north, symmetric, at the library's radang in single precision; 96 columns 3.75 degrees apart
    from 0; the area of a row is the library's Gaussian weight over its 96 points."""
    n = hip_lib.spd_get_table_host(None, b"radang", None, 0)
    radang = np.empty(n)
    hip_lib.spd_get_table_host(None, b"radang", radang.ctypes.data_as(C.c_void_p), n)
    assert pw.lat.shape == (48,) and pw.lon.shape == (96,) and pw.area.shape == (48, 96)
    assert (np.diff(pw.lat) > 0).all() and pw.lat[0] < -87.0 and pw.lat[-1] > 87.0
    assert np.array_equal(pw.lat, -pw.lat[::-1])
    assert np.array_equal(pw.lat, (radang.astype(np.float32) * np.float32(90.0) / np.arcsin(np.float32(1.0))).astype(np.float64))
    assert pw.lon.tolist() == [3.75 * i for i in range(96)]
    assert np.array_equal(pw.area, pw.area[::-1]) and (pw.area > 0).all() and (pw.area == pw.area[:, :1]).all()
    assert pw.area[0, 0] < pw.area[23, 0]  # (the polar rows weigh least)
    assert abs(pw.area.sum() - 1.0) < 1e-14


def test_every_map_sums_to_one(pw):
    maps = {"global": pw.global_mean(), "nino34": pw.box(190.0, 240.0, -5.0, 5.0), "date line": pw.box(170.0, -170.0, -30.0, 30.0),
            "band": pw.band(30.0, 60.0), "point": pw.point(11.3, 47.9), "south of the grid": pw.point(359.0, -89.9),
            "north of the grid": pw.point(-0.5, 90.0)}
    for name, w in maps.items():
        assert w.shape == (48, 96) and w.dtype == np.float64 and np.isfinite(w).all() and (w >= 0).all(), name
        assert ulps_from_one(w) <= 4.0, (name, ulps_from_one(w))
    assert int((maps["nino34"] > 0).sum()) == 14 * 2  # 191.25 ... 240 in 14 columns, the two rows at +-1.86 degrees
    assert int((maps["point"] > 0).sum()) == 4


def test_box_band_and_global_mean(pw):
    g = pw.global_mean()
    assert np.array_equal(pw.box(0.0, 360.0, -90.0, 90.0), g) and np.array_equal(pw.band(-90.0, 90.0), g)
    assert np.array_equal(pw.box(-180.0, 180.0, -90.0, 90.0), g)
    assert (g > 0).all() and np.allclose(g, pw.area, rtol=1e-14, atol=0.0)
    # inside a box the weights are proportional to the area, outside they are zero
    box = pw.box(100.0, 130.0, 10.0, 50.0)
    inside = (pw.lon[None, :] >= 100.0) & (pw.lon[None, :] <= 130.0) & (pw.lat[:, None] >= 10.0) & (pw.lat[:, None] <= 50.0)
    assert np.array_equal(box > 0, inside) and inside.sum() == 8 * 10
    assert np.array_equal(box, np.where(inside, pw.area, 0.0) / math.fsum(np.where(inside, pw.area, 0.0).ravel()))
    band = pw.band(-20.0, 20.0)
    assert np.array_equal(band > 0, np.broadcast_to((np.abs(pw.lat) <= 20.0)[:, None], (48, 96)))
    # a box across the date line is the union of its two halves, renormalised
    whole, west, east = pw.box(150.0, 210.0, -40.0, 25.0), pw.box(150.0, 180.0, -40.0, 25.0), pw.box(183.75, 210.0, -40.0, 25.0)
    union = (west > 0) | (east > 0)
    assert not ((west > 0) & (east > 0)).any() and union.sum() == 17 * 18
    assert np.array_equal(whole, np.where(union, pw.area, 0.0) / math.fsum(np.where(union, pw.area, 0.0).ravel()))
    assert np.array_equal(pw.box(150.0, -150.0, -40.0, 25.0), whole) and np.array_equal(pw.box(-210.0, -150.0, -40.0, 25.0), whole)
    # ... and across the grid's own seam at 0 degrees
    seam = pw.box(350.0, 10.0, 0.0, 90.0)
    assert np.array_equal((seam > 0).any(axis=0), (pw.lon >= 350.0) | (pw.lon <= 10.0)) and (seam > 0).any(axis=0).sum() == 5
    for args in ((10.0, 11.0, -5.0, 5.0), (0.0, 360.0, 0.1, 0.2), (0.0, 360.0, 88.0, 90.0)):
        with pytest.raises(ValueError, match="holds no grid point"):
            pw.box(*args)


def test_point(pw):
    # at a grid point: weight 1 there, nothing else
    for j, i in ((0, 0), (20, 95), (47, 13)):
        w = pw.point(pw.lon[i], pw.lat[j])
        assert w[j, i] == 1.0 and np.count_nonzero(w) == 1, (j, i)
        assert np.array_equal(pw.point(pw.lon[i] - 720.0, pw.lat[j]), w)
    # between grid points: a field linear in longitude and in latitude index is reproduced to rounding
    jj, ii = np.meshgrid(np.arange(48.0), np.arange(96.0), indexing="ij")
    field = 3.0 + 0.25 * pw.lon[None, :] + 1.5 * jj + 0.0 * ii
    for lon, j0, fy in ((11.3, 30, 0.3), (200.0 + 1.0 / 3.0, 0, 0.9), (93.7, 46, 0.5), (3.0, 23, 0.125)):
        lat = pw.lat[j0] + fy * (pw.lat[j0 + 1] - pw.lat[j0])
        w = pw.point(lon, lat)
        assert np.count_nonzero(w) == 4 and (w >= 0).all()
        expected = 3.0 + 0.25 * lon + 1.5 * (j0 + fy)
        assert abs(float(np.sum(w * field)) - expected) <= 1e-12 * abs(expected), (lon, lat)
    # periodic in longitude: between the last column and the first
    w = pw.point(358.125, pw.lat[10])
    assert w[10, 95] == 0.5 and w[10, 0] == 0.5 and np.count_nonzero(w) == 2
    # clamped in latitude to the outermost rows
    assert np.array_equal(pw.point(30.0, -90.0), pw.point(30.0, pw.lat[0])) and pw.point(30.0, -90.0)[0, 8] == 1.0
    assert np.array_equal(pw.point(30.0, 89.0), pw.point(30.0, pw.lat[47])) and pw.point(30.0, 89.0)[47, 8] == 1.0


def test_climate_indices_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("climate_indices", os.path.join(ROOT, "examples", "climate_indices.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.days) == (8, 10)
    args = mod.parse(["--members", "16", "--days", "30"])
    assert (args.members, args.days) == (16, 30)
    assert mod.EVERY == 36 and mod.LEVELS_HPA == (500.0,)
    assert [e[0] for e in mod.INDICES] == ["t_low_global", "precip_global", "nino34", "mslp_azores", "mslp_iceland", "z500_station"]
    with pytest.raises(SystemExit):
        mod.parse(["--members", "1"])
    with pytest.raises(SystemExit):
        mod.parse(["--days", "0"])
    with pytest.raises(SystemExit):
        mod.parse(["--help"])
