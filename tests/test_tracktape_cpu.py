"""CPU tier: the track tape's entry points (spd_model_tracktape_*, spd_track_point_host) are declared, exported and bound; the
argument checks the library makes before it needs a model or a device, in their documented order; the rule for one plane --
spd_track_point_host, the host compile of the routines the kernel runs (csrc/track_point.hpp) -- bitwise against the numpy
restatement (tests/tracktape_reference.py), and that against a loop over Python floats, on synthetic planes built to take every
branch; EnsembleModel.tracktape_lonlat; the storm-track example parses its arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import tracktape_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKTAPE_SYMBOLS = ("spd_model_tracktape_configure", "spd_model_tracktape_reset", "spd_model_tracktape_info", "spd_model_tracktape_times",
                     "spd_model_tracktape_read", "spd_model_tracktape_positions", "spd_model_tracktape_seed", "spd_track_point_host")
FOURTEEN = b"(u_grid, v_grid, t_grid, q_grid, phi_grid, ps_grid, precnv, precls, u_plev, v_plev, t_plev, q_plev, z_plev, mslp)"
IX, IL, POINTS = 96, 48, 4608


def test_tracktape_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in TRACKTAPE_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for method in ("tracktape_configure", "tracktape_off", "tracktape_reset", "tracktape_info", "tracktape_entries", "tracktape_steps",
                   "tracktape_times", "tracktape", "tracktape_positions", "tracktape_seed", "tracktape_lonlat"):
        assert hasattr(EnsembleModel, method), method
    assert isinstance(EnsembleModel.tracktape_info, property) and isinstance(EnsembleModel.tracktape_entries, property)
    # the constants agree: header, Fortran, _lib, the reference and the Python names
    assert "#define SPD_TRACK_MIN 0\n" in header and "#define SPD_TRACK_MAX 1\n" in header
    assert "SPD_TRACK_MIN = 0, SPD_TRACK_MAX = 1" in fortran
    assert (L.SPD_TRACK_MIN, L.SPD_TRACK_MAX) == (0, 1) == (ref.MIN, ref.MAX)
    assert EnsembleModel.TRACK_OPS == {"min": 0, "max": 1}


# ---- the argument checks that need neither a model nor a device --------------------------------------------------------
def _call(hip_lib, regions, n_regions, rows, every, capacity, n_entries=None, arrays=True):
    n = max(len(rows), 1)
    names = (C.c_char_p * n)(*[r[0].encode() for r in rows])
    columns = [(C.c_int * n)(*[r[k] for r in rows]) for k in (1, 2, 3, 4)]
    w = None if regions is None else np.ascontiguousarray(regions, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    if not arrays:
        names, columns = None, [None] * 4
    return hip_lib.spd_model_tracktape_configure(None, w, n_regions, names, *columns, len(rows) if n_entries is None else n_entries, every,
                                                 capacity)


ONES = np.ones((2, 48, 96))
NAN_AT = ONES.copy()
NAN_AT[1, 3, 5] = np.nan  # region 1, point 96 * 3 + 5 = 293
EMPTY = ONES.copy()
EMPTY[1] = 0.0
OK = ("t_grid", 7, 0, 0, 2)


@pytest.mark.parametrize("regions, n_regions, rows, every, capacity, message", [
    (ONES, 2, (OK,), 0, 4, b"every must be at least 1"),
    (ONES, 2, (OK,), 3, 0, b"capacity must be at least 1"),
    (ONES, 0, (OK,), 3, 4, b"n_regions must be 1 ... 64, got 0"),
    (ONES, 65, (OK,), 3, 4, b"n_regions must be 1 ... 64, got 65"),
    (None, 2, (OK,), 3, 4, b"null regions"),
    (NAN_AT, 2, (OK,), 3, 4, b"weight of pattern 1 at point 293 (row 3, column 5) is not finite"),
    (EMPTY, 2, (OK,), 3, 4, b"region 1 holds no point"),
    (ONES, 2, (OK, ("olr", 0, 0, 0, 0)), 3, 4, b"unknown variable 'olr' " + FOURTEEN),
    (ONES, 2, (("t_grid", 8, 0, 0, 0),), 3, 4, b"level 8 of entry 0 ('t_grid') is out of range (0 ... 7)"),
    (ONES, 2, (OK, ("mslp", 1, 0, 0, 0)), 3, 4, b"level 1 of entry 1 ('mslp') is out of range (0 ... 0)"),
    (ONES, 2, (("z_plev", -1, 0, 0, 0),), 3, 4, b"level -1 of entry 0 ('z_plev') is out of range"),
    (ONES, 2, (("t_grid", 0, 2, 0, 0),), 3, 4, b"pattern 2 of entry 0 ('t_grid') is out of range (0 ... 1)"),
    (ONES, 2, (OK, ("ps_grid", 0, -1, 0, 0)), 3, 4, b"pattern -1 of entry 1 ('ps_grid') is out of range (0 ... 1)"),
    (ONES, 2, (("t_grid", 0, 1, 2, 0),), 3, 4, b"op 2 of entry 0 ('t_grid') is not SPD_TRACK_MIN (0) or SPD_TRACK_MAX (1)"),
    (ONES, 2, (OK, ("tcwv", 0, 1, -1, 0)), 3, 4, b"op -1 of entry 1 ('tcwv') is not SPD_TRACK_MIN (0) or SPD_TRACK_MAX (1)"),
    (ONES, 2, (("t_grid", 0, 1, 1, 25),), 3, 4, b"radius 25 of entry 0 ('t_grid') is out of range (0 ... 24)"),
    (ONES, 2, (("t_grid", 0, 1, 1, -1),), 3, 4, b"radius -1 of entry 0 ('t_grid') is out of range (0 ... 24)"),
    # (the same plane under two regions and both ops, radius 24, a derived and a pressure-level name are fine until a model is needed)
    (ONES, 2, (OK, ("t_grid", 7, 1, 1, 24), ("t_grid", 7, 1, 1, 24), ("z_plev", 11, 0, 0, 0), ("tcwv", 0, 0, 1, 0)), 3, 4, b"null model"),
])
def test_configure_checks_its_arguments_first(hip_lib, regions, n_regions, rows, every, capacity, message):
    assert _call(hip_lib, regions, n_regions, rows, every, capacity) == -1
    assert message in hip_lib.spd_last_error(), hip_lib.spd_last_error()
    assert b"spd_model_tracktape_configure" in hip_lib.spd_last_error()


def test_argument_checks_come_in_the_documented_order(hip_lib):
    """every, capacity, n_regions, n_entries, null regions, null lists, a weight that is not finite, an empty region, an unknown
    name, per entry its level, its region, its op and then its radius, then the null model: each case is wrong in everything that
    comes later as well."""
    bad = (("olr", 9, 9, 9, 99), ("t_grid", 9, 9, 9, 99))
    both = np.stack([NAN_AT[1], EMPTY[1]])  # one weight not finite AND an empty region
    cases = [(dict(regions=None, n_regions=0, rows=bad, every=0, capacity=0, n_entries=2000, arrays=False), b"every must"),
             (dict(regions=None, n_regions=0, rows=bad, every=1, capacity=0, n_entries=2000, arrays=False), b"capacity must"),
             (dict(regions=None, n_regions=0, rows=bad, every=1, capacity=1, n_entries=2000, arrays=False), b"n_regions must"),
             (dict(regions=None, n_regions=2, rows=bad, every=1, capacity=1, n_entries=2000, arrays=False), b"n_entries must be 0 ... 1024, got 2000"),
             (dict(regions=None, n_regions=2, rows=bad, every=1, capacity=1, n_entries=-1, arrays=False), b"n_entries must be 0 ... 1024, got -1"),
             (dict(regions=None, n_regions=2, rows=bad, every=1, capacity=1, arrays=False), b"null regions"),
             (dict(regions=both, n_regions=2, rows=bad, every=1, capacity=1, arrays=False), b"bad list of entries"),
             (dict(regions=both, n_regions=2, rows=bad, every=1, capacity=1), b"is not finite"),
             (dict(regions=EMPTY, n_regions=2, rows=bad, every=1, capacity=1), b"region 1 holds no point"),
             (dict(regions=ONES, n_regions=2, rows=bad, every=1, capacity=1), b"unknown variable 'olr'"),
             (dict(regions=ONES, n_regions=2, rows=bad[1:], every=1, capacity=1), b"level 9 of entry 0"),
             (dict(regions=ONES, n_regions=2, rows=(("t_grid", 0, 9, 9, 99), ("t_grid", 9, 0, 0, 0)), every=1, capacity=1), b"pattern 9 of entry 0"),
             (dict(regions=ONES, n_regions=2, rows=(("t_grid", 0, 1, 9, 99),), every=1, capacity=1), b"op 9 of entry 0"),
             (dict(regions=ONES, n_regions=2, rows=(("t_grid", 0, 1, 1, 99),), every=1, capacity=1), b"radius 99 of entry 0"),
             (dict(regions=ONES, n_regions=2, rows=(("t_grid", 0, 1, 1, 24),), every=1, capacity=1), b"null model")]
    for kw, message in cases:
        assert _call(hip_lib, **kw) == -1
        assert message in hip_lib.spd_last_error(), (message, hip_lib.spd_last_error())


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    buf = C.c_double()
    taken, held = C.c_longlong(), C.c_int()
    rows = (C.c_int32 * 6)()
    # switching off looks at nothing but the model
    assert hip_lib.spd_model_tracktape_configure(None, None, 0, None, None, None, None, None, 0, 0, 0) == -1
    assert b"spd_model_tracktape_configure: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tracktape_reset(None) == -1 and b"spd_model_tracktape_reset: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tracktape_info(None, C.byref(taken), C.byref(held), None, None, None, None) == -1
    assert b"spd_model_tracktape_info: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tracktape_times(None, rows, 1) == -1 and b"spd_model_tracktape_times: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tracktape_read(None, 0, 1, 0, 1, C.byref(buf), 8, None) == -1
    assert b"spd_model_tracktape_read: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tracktape_positions(None, 0, 1, rows, 6) == -1
    assert b"spd_model_tracktape_positions: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_tracktape_seed(None, 0, 1, rows) == -1 and b"spd_model_tracktape_seed: null model" in hip_lib.spd_last_error()


# ---- the rule for one plane: the library's host compile, numpy, Python floats ----------------------------------------------
def base_plane():
    """4608 distinct values, exactly representable: 100 + a permutation of 0 ... 4607 eighths (7919 is prime to 4608); the same
    recipe as tests/sanitize/tracktape_sanitize.cpp"""
    p = np.arange(POINTS)
    return (100.0 + ((p * 7919) % POINTS) * 0.125).reshape(IL, IX)


def box_mask(j0, j1, i0, i1):
    """rows j0 ... j1 and columns i0 ... i1, both ends included; i0 > i1 wraps"""
    m = np.zeros((IL, IX), dtype=np.uint8)
    cols = np.arange(IX)
    m[j0:j1 + 1, (cols >= i0) & (cols <= i1) if i0 <= i1 else (cols >= i0) | (cols <= i1)] = 1
    return m


ALL = np.ones((IL, IX), dtype=np.uint8)


def with_points(points, plane=None):
    x = base_plane() if plane is None else plane.copy()
    for (j, i), v in points.items():
        x[j, i] = v
    return x


def at(j, i):
    return float(IX * j + i)


INF = float("inf")
# name: (plane, mask, prev, radius, op, expected (value, p, di, dj) or None where only the three implementations are compared)
CASES = {
    # the tie goes to the first region point, both denominators are 0
    "constant": (np.full((IL, IX), 5.0), box_mask(10, 20, 30, 40), -1, 0, ref.MIN, (5.0, at(10, 30), 0.0, 0.0)),
    "constant max": (np.full((IL, IX), 5.0), box_mask(10, 20, 90, 3), -1, 0, ref.MAX, (5.0, at(10, 0), 0.0, 0.0)),
    # the winner in column 0 and in column 95: a neighbour wraps.  a = 200, b = 0, c = 100: den 300, num 50
    "column 0": (with_points({(20, 0): 0.0, (20, 95): 200.0, (20, 1): 100.0, (19, 0): 50.0, (21, 0): 50.0}), ALL, -1, 0, ref.MIN,
                 (0.0, at(20, 0), 50.0 / 300.0, 0.0)),
    "column 95": (with_points({(20, 95): 0.0, (20, 94): 100.0, (20, 0): 200.0, (19, 95): 50.0, (21, 95): 150.0}), ALL, -1, 0, ref.MIN,
                  (0.0, at(20, 95), -50.0 / 300.0, -50.0 / 200.0)),
    # rows 0 and 47: dj = 0
    "row 0": (with_points({(0, 50): 0.0, (0, 49): 64.0, (0, 51): 32.0}), ALL, -1, 0, ref.MIN, (0.0, at(0, 50), 16.0 / 96.0, 0.0)),
    "row 47": (with_points({(47, 50): 5000.0, (47, 49): 4000.0, (47, 51): 4500.0}), ALL, -1, 0, ref.MAX,
               (5000.0, at(47, 50), 0.5 * (4000.0 - 4500.0) / ((4000.0 - 10000.0) + 4500.0), 0.0)),
    # a neighbour outside the region more extreme than the winner: den = (-10 - 0) + 200 = 190, num = -105, the quotient is clamped
    # and (300 - 0) - 20 = 280, num = 160 likewise
    "clamp": (with_points({(20, 10): 0.0, (20, 9): -10.0, (20, 11): 200.0, (19, 10): 300.0, (21, 10): -20.0}), box_mask(20, 20, 10, 12), -1, 0,
              ref.MIN, (0.0, at(20, 10), -0.5, 0.5)),
    # NaN inside the region never wins, and a NaN neighbour leaves the offset 0
    "nan in the region": (with_points({(12, 33): np.nan, (12, 34): 1.0, (13, 34): 3.0, (11, 34): 4.0, (12, 35): 2.0}), box_mask(10, 20, 30, 40),
                          -1, 0, ref.MIN, (1.0, at(12, 34), 0.0, 0.5 * (4.0 - 3.0) / ((4.0 - 2.0) + 3.0))),
    "nan in the region, max": (with_points({(12, 33): np.nan}), box_mask(10, 20, 30, 40), -1, 0, ref.MAX, None),
    "all nan": (with_points({(j, i): np.nan for j in range(10, 13) for i in range(30, 33)}), box_mask(10, 12, 30, 32), -1, 0, ref.MIN,
                (np.nan, -1.0, 0.0, 0.0)),
    "all nan, followed": (with_points({(j, i): np.nan for j in range(10, 13) for i in range(30, 33)}), box_mask(10, 12, 30, 32), 96 * 11 + 31, 1,
                          ref.MAX, (np.nan, -1.0, 0.0, 0.0)),
    # infinities compare as numbers; their offsets are 0 (den is not finite)
    "-inf wins": (with_points({(5, 5): -INF}), ALL, -1, 0, ref.MIN, (-INF, at(5, 5), 0.0, 0.0)),
    "+inf wins": (with_points({(5, 5): INF, (40, 7): INF}), ALL, -1, 0, ref.MAX, (INF, at(5, 5), 0.0, 0.0)),
    "+inf loses": (with_points({(5, 5): INF, (30, 30): 0.0, (30, 29): INF, (29, 30): 1.0, (31, 30): 2.0}), ALL, -1, 0, ref.MIN,
                   (0.0, at(30, 30), 0.0, 0.5 * (1.0 - 2.0) / ((1.0 - 0.0) + 2.0))),
    # the two zeros are equal values: the lower index wins and keeps its sign
    "zeros": (with_points({(5, 5): 0.0, (10, 10): -0.0}, np.full((IL, IX), 1.0)), ALL, -1, 0, ref.MIN, (0.0, at(5, 5), 0.0, 0.0)),
    "zeros, minus first": (with_points({(5, 5): -0.0, (10, 10): 0.0}, np.full((IL, IX), -1.0)), ALL, -1, 0, ref.MAX, (-0.0, at(5, 5), -0.0, -0.0)),
    # a window across the date line: column 94 is 3 from column 1, column 93 is 4
    "date line": (with_points({(20, 50): -1000.0, (21, 93): -700.0, (21, 94): -500.0, (17, 2): -400.0}), ALL, 96 * 20 + 1, 3, ref.MIN, None),
    # a window clipped at a pole row: rows 0 ... 6 of a radius-5 window round row 1
    "pole": (with_points({(7, 40): -1000.0, (0, 38): -500.0, (6, 45): -400.0, (1, 46): -900.0}), ALL, 96 * 1 + 40, 5, ref.MIN, None),
    "north pole, max": (with_points({(41, 3): 9000.0, (47, 95): 8000.0, (42, 90): 7000.0}), ALL, 96 * 46 + 0, 4, ref.MAX, None),
    # radius 24: rows 0 ... 47 and columns 24 ... 72 round (24, 48)
    "radius 24": (with_points({(3, 73): -1000.0, (47, 23): -900.0, (47, 24): -500.0, (0, 72): -400.0}), ALL, 96 * 24 + 48, 24, ref.MIN, None),
    # prev = -1 with radius > 0: the whole region
    "not seeded": (with_points({(20, 50): -1000.0, (21, 94): -500.0}), ALL, -1, 3, ref.MIN, None),
    # radius 0 never follows, whatever prev says
    "radius 0": (with_points({(20, 50): -1000.0, (21, 94): -500.0}), ALL, 96 * 20 + 1, 0, ref.MIN, None),
    # a window and a region that share a few points only
    "window and box": (base_plane(), box_mask(18, 30, 90, 5), 96 * 20 + 1, 3, ref.MAX, None),
}
WINNERS = {"date line": at(21, 94), "pole": at(0, 38), "north pole, max": at(47, 95), "radius 24": at(47, 24), "not seeded": at(20, 50),
           "radius 0": at(20, 50)}


def host(hip_lib, plane, mask, prev, radius, op):
    x = np.ascontiguousarray(plane, dtype=np.float64)
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    out = np.full(4, -7.0)
    rc = hip_lib.spd_track_point_host(x.ctypes.data_as(C.POINTER(C.c_double)), m.ctypes.data_as(C.POINTER(C.c_ubyte)), prev, radius, op,
                                      out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, hip_lib.spd_last_error()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_host_routine_numpy_and_python_floats_agree_bitwise(hip_lib, case):
    plane, mask, prev, radius, op, expected = CASES[case]
    numpy_, loop, lib = ref.track(plane, mask, prev, radius, op), ref.track_loop(plane, mask, prev, radius, op), host(hip_lib, plane, mask, prev, radius, op)
    print(case, [float(v) for v in numpy_])
    assert ref.bits(numpy_) == ref.bits(loop), (case, numpy_, loop)
    assert ref.bits(lib) == ref.bits(numpy_), (case, lib.tolist(), numpy_)
    if expected is not None:
        assert ref.bits(numpy_) == ref.bits(expected), (case, numpy_, expected)
    if case in WINNERS:
        assert float(numpy_[1]) == WINNERS[case]
    if case == "clamp":  # the unclamped quotients lie outside, away from a zero denominator
        assert -105.0 / 190.0 < -0.5 and 0.5 * (300.0 + 20.0) / ((300.0 - 0.0) - 20.0) > 0.5


def test_the_rule_on_random_planes_and_regions(hip_lib):
    """Seeded random planes with ties, NaN and infinities sprinkled in, random boxes, both ops, seeded and not: the three
    implementations agree bitwise, the winner is a candidate no other candidate beats, and some offset lies strictly inside."""
    rng = np.random.default_rng(11)
    inside = 0
    for k in range(40):
        x = np.round(rng.normal(0.0, 3.0, (IL, IX)), 1 if k % 2 else 6)  # (one decimal: many ties)
        for v in (np.nan, np.inf, -np.inf):
            x[rng.integers(0, IL, 3), rng.integers(0, IX, 3)] = v
        j0, i0 = int(rng.integers(0, IL)), int(rng.integers(0, IX))
        mask = box_mask(j0, min(IL - 1, j0 + int(rng.integers(0, 20))), i0, (i0 + int(rng.integers(0, 60))) % IX)
        region = np.flatnonzero(mask.ravel())
        prev = int(rng.choice(region)) if k % 3 else -1
        radius, op = int(rng.integers(0, 25)), k % 2
        numpy_ = ref.track(x, mask, prev, radius, op)
        assert ref.bits(numpy_) == ref.bits(ref.track_loop(x, mask, prev, radius, op)), k
        assert ref.bits(host(hip_lib, x, mask, prev, radius, op)) == ref.bits(numpy_), k
        cand = (mask.ravel() != 0) & ~np.isnan(x.ravel())
        if radius > 0 and prev >= 0:
            cand &= ref.window(prev, radius)
        p = int(numpy_[1])
        if p < 0:
            assert not cand.any()
            continue
        assert cand[p] and x.ravel()[p] == (x.ravel()[cand].max() if op else x.ravel()[cand].min())
        assert not (cand[:p] & (x.ravel()[:p] == x.ravel()[p])).any()
        inside += sum(1 for d in numpy_[2:] if d != 0.0 and abs(d) < 0.5)
    assert inside >= 10


def test_host_routine_checks_its_arguments(hip_lib):
    x, m, out = np.zeros(POINTS), np.ones(POINTS, dtype=np.uint8), np.zeros(4)
    px, pm, po = x.ctypes.data_as(C.POINTER(C.c_double)), m.ctypes.data_as(C.POINTER(C.c_ubyte)), out.ctypes.data_as(C.POINTER(C.c_double))
    for args, message in (((None, pm, -1, 0, 0, po), b"null argument"), ((px, None, -1, 0, 0, po), b"null argument"),
                          ((px, pm, -1, 0, 0, None), b"null argument"), ((px, pm, -2, 0, 0, po), b"prev must be -1 or 0 ... 4607, got -2"),
                          ((px, pm, 4608, 0, 0, po), b"prev must be -1 or 0 ... 4607, got 4608"), ((px, pm, -1, 25, 0, po), b"radius must be 0 ... 24, got 25"),
                          ((px, pm, -1, -1, 0, po), b"radius must be 0 ... 24, got -1"), ((px, pm, -1, 0, 2, po), b"op must be SPD_TRACK_MIN or SPD_TRACK_MAX, got 2")):
        assert hip_lib.spd_track_point_host(*args) == -1
        assert message in hip_lib.spd_last_error(), hip_lib.spd_last_error()


def test_follow_carries_the_position(hip_lib):
    """A low that moves two columns a sample is followed with radius 2 while a deeper one appears elsewhere; with radius 0 the
    deeper one is taken at once."""
    planes = []
    for s in range(5):
        x = base_plane()
        x[30, (94 + 2 * s) % IX] = -10.0  # crosses the seam of the grid
        if s >= 2:
            x[10, 40] = -20.0
        planes.append(x)
    followed, last = ref.follow(planes, ALL, 2, ref.MIN)
    free, _ = ref.follow(planes, ALL, 0, ref.MIN)
    assert followed[:, 1].tolist() == [at(30, 94), at(30, 0), at(30, 2), at(30, 4), at(30, 6)] and last == 96 * 30 + 6
    assert free[:, 1].tolist() == [at(30, 94), at(30, 0), at(10, 40), at(10, 40), at(10, 40)]


def test_lonlat(hip_lib):
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel
    lat = pyspeedy_amd.projection_weights().lat
    track = np.array([[1.0, at(20, 0), -0.25, 0.5], [1.0, at(0, 95), 0.5, 0.0], [1.0, at(47, 10), 0.0, 0.0], [1.0, at(30, 8), 0.0, -0.5],
                      [np.nan, -1.0, 0.0, 0.0]])
    lon, la = EnsembleModel.tracktape_lonlat(track)
    assert lon[:4].tolist() == [360.0 - 0.9375, 3.75 * 95.5, 37.5, 30.0] and np.isnan(lon[4]) and np.isnan(la[4])
    assert la[:4].tolist() == [lat[20] + 0.5 * (lat[21] - lat[20]), lat[0], lat[47], lat[30] + 0.5 * (lat[29] - lat[30])]
    assert EnsembleModel.tracktape_lonlat(track.reshape(1, 5, 4))[0].shape == (1, 5)


def test_storm_track_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("storm_track", os.path.join(ROOT, "examples", "storm_track.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.days) == (8, 5)
    args = mod.parse(["--members", "16", "--days", "10"])
    assert (args.members, args.days) == (16, 10)
    assert mod.EVERY == 9 and mod.RADIUS == 2 and mod.BOX == (280.0, 350.0, 30.0, 70.0)
    with pytest.raises(SystemExit):
        mod.parse(["--members", "0"])
    with pytest.raises(SystemExit):
        mod.parse(["--days", "0"])
    with pytest.raises(SystemExit):
        mod.parse(["--help"])
