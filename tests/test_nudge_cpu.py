"""CPU tier: the nudging entry points (spd_model_nudge_*) are declared, exported and bound; the argument checks the library makes
before it needs a model or a device, in their documented order; pyspeedy_amd.nudge_gains against its formula; the nudged-replay
example parses its arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUDGE_SYMBOLS = ("spd_model_nudge_configure", "spd_model_nudge_set_times", "spd_model_nudge_set_target", "spd_model_nudge_apply",
                 "spd_model_nudge_info")
NAN, INF = float("nan"), float("inf")


def test_nudge_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd
    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in NUDGE_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for method in ("nudge_configure", "nudge_targets", "nudge_apply", "nudge_info", "nudge_off"):
        assert hasattr(EnsembleModel, method), method
    assert EnsembleModel.NUDGE_NAMES == ("vor", "div", "t", "tr", "ps")
    assert pyspeedy_amd.nudge_gains is L.nudge_gains and "nudge_gains" in pyspeedy_amd.__all__


def _configure(hip_lib, names, gains, capacity=2, in_loop=1, n=None, mask=None):
    """spd_model_nudge_configure on a null model; gains: None, or {(name index, level, l): value} over a table of 0.5"""
    arr = None if names is None else (C.c_char_p * max(len(names), 1))(*[s if s is None else s.encode() for s in names])
    table = None
    if gains is not None:
        t = np.full((max(len(names or ()), 1), 8, 32), 0.5)
        for at, value in gains.items():
            t[at] = value
        table = t.ctypes.data_as(C.POINTER(C.c_double))
    rc = hip_lib.spd_model_nudge_configure(None, arr, len(names or ()) if n is None else n, table, mask, capacity, in_loop)
    return rc, hip_lib.spd_last_error()


@pytest.mark.parametrize("names, gains, capacity, in_loop, n, message", [
    (None, {}, 2, 1, 2, b"bad list of names"),
    (["vor"], {}, 2, 1, -1, b"bad list of names"),
    (["vor", "div", "t", "tr", "ps", "vor"], {}, 2, 1, None, b"bad list of names"),  # (more than five)
    (["vor", "phi"], {}, 2, 1, None, b"unknown variable 'phi' (vor, div, t, tr, ps)"),
    (["t_grid"], {}, 2, 1, None, b"unknown variable 't_grid' (vor, div, t, tr, ps)"),
    ([None], {}, 2, 1, None, b"unknown variable '(null)'"),
    (["vor", "t", "vor"], {}, 2, 1, None, b"'vor' named twice"),
    (["vor", "t"], None, 2, 1, None, b"null gains"),
    (["vor", "t"], {(1, 3, 17): 1.0000001}, 2, 1, None, b"the gain of 't' at level 3, wavenumber 17 is not a finite number in [0, 1]"),
    (["vor", "t"], {(0, 7, 31): -1e-300}, 2, 1, None, b"the gain of 'vor' at level 7, wavenumber 31 is not"),
    (["div"], {(0, 0, 0): NAN}, 2, 1, None, b"the gain of 'div' at level 0, wavenumber 0 is not"),
    (["tr"], {(0, 2, 5): INF}, 2, 1, None, b"the gain of 'tr' at level 2, wavenumber 5 is not"),
    (["ps"], {(0, 0, 9): 2.0}, 2, 1, None, b"the gain of 'ps' at level 0, wavenumber 9 is not"),
    (["vor"], {}, 0, 1, None, b"capacity must be at least 1"),
    (["vor"], {}, 1, 2, None, b"in_loop must be 0 or 1"),
    (["vor"], {}, 1, -1, None, b"in_loop must be 0 or 1"),
    # (the rows of ps behind its first are not gains: never read, never refused; 0 and 1 are gains)
    (["ps", "vor"], {(0, 1, 0): 7.0, (1, 0, 0): 0.0, (1, 7, 31): 1.0}, 1, 0, None, b"null model"),
])
def test_configure_checks_its_arguments_first(hip_lib, names, gains, capacity, in_loop, n, message):
    rc, text = _configure(hip_lib, names, gains, capacity, in_loop, n)
    assert rc == -1
    assert message in text, text
    assert b"spd_model_nudge_configure" in text


def test_argument_checks_come_in_the_documented_order(hip_lib):
    """bad list, unknown name, name twice, null gains, a gain out of [0, 1], capacity, in_loop, then the null model: each case is
    wrong in everything that comes later as well."""
    bad_mask = (C.c_int32 * 4)(1, 0, 7, 1)  # (a mask entry other than 0 / 1 comes after the model, which is never there)
    cases = [(["olr", "olr"], None, 0, 7, b"unknown variable"),
             (["vor", "vor"], None, 0, 7, b"named twice"),
             (["vor", "div"], None, 0, 7, b"null gains"),
             (["vor", "div"], {(1, 4, 20): 1.5}, 0, 7, b"the gain of 'div' at level 4, wavenumber 20"),
             (["vor", "div"], {}, 0, 7, b"capacity must"),
             (["vor", "div"], {}, 3, 7, b"in_loop must"),
             (["vor", "div"], {}, 3, 1, b"null model")]
    for names, gains, capacity, in_loop, message in cases:
        rc, text = _configure(hip_lib, names, gains, capacity, in_loop, mask=bad_mask)
        assert rc == -1 and message in text, (message, text)
    # the list itself comes before everything else
    rc, text = _configure(hip_lib, ["olr"] * 6, None, 0, 7)
    assert rc == -1 and b"bad list of names" in text
    # switching off looks at nothing but the list, and still needs a model
    rc, text = _configure(hip_lib, None, None, 0, 7, n=0)
    assert rc == -1 and b"spd_model_nudge_configure: null model" in text


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    steps = (C.c_int32 * 3)(3, 5, 9)
    field = np.zeros(992 * 8, dtype=np.complex128)
    n, applied = C.c_int(), C.c_longlong()
    assert hip_lib.spd_model_nudge_set_times(None, steps, 3) == -1
    assert b"spd_model_nudge_set_times: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_nudge_set_times(None, None, 3) == -1 and b"bad list of steps" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_nudge_set_times(None, (C.c_int32 * 3)(3, 3, 9), 3) == -1
    assert b"strictly ascending (slot 1)" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_nudge_set_target(None, 0, b"t", field.ctypes.data_as(C.c_void_p), field.nbytes) == -1
    assert b"spd_model_nudge_set_target: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_nudge_set_target(None, 0, b"phi", field.ctypes.data_as(C.c_void_p), field.nbytes) == -1
    assert b"unknown variable 'phi'" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_nudge_set_target(None, 0, b"t", None, 0) == -1 and b"null argument" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_nudge_apply(None, 0, 1, None) == -1 and b"spd_model_nudge_apply: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_nudge_info(None, C.byref(n), None, None, None, C.byref(applied)) == -1
    assert b"spd_model_nudge_info: null model" in hip_lib.spd_last_error()


# ---- the gain table ------------------------------------------------------------------------------------------------------
def weight(l, l_max, taper):
    """the definition, coefficient by coefficient"""
    if l <= l_max - taper:
        return 1.0
    if l >= l_max + 1:
        return 0.0
    return (l_max + 1 - l) / (taper + 1.0)


@pytest.mark.parametrize("tau, l_max, taper", [(6.0, 31, 0), (6.0, 15, 0), (24.0, 15, 5), (2.0 / 3.0, 20, 20), (48.0, 40, 12), (1.0, 0, 0),
                                               (3.0, 31, 31)])
def test_nudge_gains_agree_with_the_formula(tau, l_max, taper):
    from pyspeedy_amd import nudge_gains
    g = nudge_gains(tau, l_max=l_max, taper=taper)
    assert g.shape == (8, 32) and g.dtype == np.float64
    want = np.array([(2400.0 / (3600.0 * tau)) * weight(l, l_max, taper) for l in range(32)])
    assert np.allclose(g, want[None, :], rtol=1e-15, atol=0.0)
    assert (g >= 0).all() and (g <= 1).all()
    # the taper's ends: full weight up to l_max - taper, nothing from l_max + 1 on, strictly between in between
    full = 2400.0 / (3600.0 * tau)
    for l in range(32):
        if l <= l_max - taper:
            assert g[0, l] == full
        elif l >= l_max + 1:
            assert g[0, l] == 0.0
        else:
            assert 0.0 < g[0, l] < full
    if l_max - taper >= 0 and l_max - taper + 1 <= min(l_max, 31):
        assert np.isclose(g[0, l_max - taper + 1], full * taper / (taper + 1.0), rtol=1e-15)


def test_nudge_gains_levels_and_refusals():
    from pyspeedy_amd import nudge_gains
    assert nudge_gains(6.0, levels=1).shape == (1, 32)  # (ps)
    per_level = nudge_gains(np.arange(1.0, 9.0), l_max=10)
    assert per_level.shape == (8, 32)
    assert np.allclose(per_level[:, 10], 2400.0 / (3600.0 * np.arange(1.0, 9.0)), rtol=1e-15) and (per_level[:, 11:] == 0).all()
    top = nudge_gains(6.0, levels=(0, 1))  # (the two stratospheric levels only)
    assert top.shape == (8, 32) and (top[:2] == 1.0 / 9.0).all() and (top[2:] == 0).all()
    assert nudge_gains(2.0 / 3.0).max() == 1.0  # (tau of exactly one step: the state is replaced by the target)
    with pytest.raises(ValueError, match="exceeds 1"):
        nudge_gains(0.5)
    with pytest.raises(ValueError, match="exceeds 1"):
        nudge_gains([6.0] * 7 + [0.6])
    with pytest.raises(ValueError, match="positive"):
        nudge_gains(0.0)
    with pytest.raises(ValueError, match="taper"):
        nudge_gains(6.0, taper=-1)


def test_nudged_replay_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("nudged_replay", os.path.join(ROOT, "examples", "nudged_replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.days, args.tau, args.l_max, args.noise) == (16, 5, 6.0, 15, 0.01)
    args = mod.parse(["--members", "64", "--days", "10", "--tau", "12", "--l-max", "10", "--noise", "0.1"])
    assert (args.members, args.days, args.tau, args.l_max, args.noise) == (64, 10, 12.0, 10, 0.1)
    assert mod.NAMES == ("vor", "div", "t") and mod.TARGET_EVERY == 9  # (six-hourly: 9 steps of 40 minutes)
    with pytest.raises(SystemExit):
        mod.parse(["--members", "1"])
    with pytest.raises(SystemExit):
        mod.parse(["--days", "0"])
    with pytest.raises(SystemExit):
        mod.parse(["--tau", "0.5"])
