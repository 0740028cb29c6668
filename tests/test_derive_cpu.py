"""CPU tier of the derived fields: pins the numpy restatement of the definitions (tests/derive_reference.py, the arbiter of
tests/test_derive_gpu.py) to the oracle's humidity scheme and to closed forms, checks the order of the argument checks that need
no model, and that the two new procedures are declared, exported and bound.  No compute entry point reaches a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import derive_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (0, 1, 2, 36, 37)


@pytest.mark.parametrize("step", STEPS)
def test_qsat_is_the_oracles_bit_for_bit(oracle, golden_dir, step):
    """The arbiter's qsat against the oracle's humidity scheme (oracle/schemes.py: OracleBackend.qsat, which test_schemes_oracle.py
    holds bitwise to the reference's) on the reference's own temperatures and pressures, every level: bit for bit
    (the arbiter takes the C library's exp, as the oracle does; with numpy's own exp the two are up to 3 ulp apart)."""
    import schemes as S
    from test_schemes_oracle import load
    inp, _ = load(golden_dir, step)
    tg, psg = inp["tg"], inp["psg"]
    fsg = oracle.table("fsg")
    for k in range(8):
        want = S.OracleBackend().qsat(np.asfortranarray(tg[:, :, k]), psg, float(fsg[k]))
        got = ref.qsat(tg[:, :, k], float(fsg[k]) * psg)
        assert want.shape == got.shape
        assert np.array_equal(got, want), (step, k, float(np.abs(got - want).max()))


def test_vertical_tables_are_the_librarys(oracle):
    assert np.array_equal(ref.FSG, np.asarray(oracle.table("fsg"), dtype=np.float64))
    assert np.array_equal(ref.DHS, np.asarray(oracle.table("dhs"), dtype=np.float64))


def test_omega_of_a_resting_column_is_exactly_zero():
    """u = v = D = 0 with any grad ln ps: every term of the continuity equation is a product with zero"""
    rng = np.random.default_rng(7)
    zero = np.zeros((8, 5, 6))
    ps = 1.0e5 * np.exp(rng.normal(0.0, 0.1, (5, 6)))
    om = ref.omega(zero, zero, zero, ps, rng.normal(0.0, 1e-6, (5, 6)), rng.normal(0.0, 1e-6, (5, 6)))
    assert om.shape == (8, 5, 6)
    assert np.array_equal(om.view(np.int64), np.zeros((8, 5, 6), dtype=np.int64))


def test_omega_of_uniform_divergence_is_linear_in_sigma():
    """u = v = 0 and the same D on every level: sigma-dot vanishes (D - Dbar = 0 to rounding) and omega[k] = -ps fsg[k] D sum(dhs)"""
    ps, d = np.full((1, 1), 98000.0), 2.0e-6
    om = ref.omega(np.zeros((8, 1, 1)), np.zeros((8, 1, 1)), np.full((8, 1, 1), d), ps, np.zeros((1, 1)), np.zeros((1, 1)))
    expect = -98000.0 * ref.FSG * d * ref.DHS.sum()
    assert np.abs(om[:, 0, 0] - expect).max() <= 1e-12 * np.abs(expect).max()


def test_column_water_of_constant_humidity():
    """tcwv of constant q is q ps sum(dhs) / g (to the rounding of eight additions)"""
    q, ps = 4.0e-3, np.array([[101325.0, 70000.0]])
    fields = {n: np.zeros((8, 1, 2)) for n in ("u", "v", "vor", "div")}
    fields["t"] = np.full((8, 1, 2), 270.0)
    fields["q"] = np.full((8, 1, 2), q)
    out = ref.derive_reference(fields, ps, np.zeros((1, 2)), np.zeros((1, 2)))
    expect = q * ps * ref.DHS.sum() / ref.GRAV
    assert np.abs(out["tcwv"] - expect).max() <= 4.0 * np.spacing(expect.max())
    assert np.array_equal(out["ivt_u"], np.zeros((1, 2))) and np.array_equal(out["ke_col"], np.zeros((1, 2)))


def test_levels_take_the_nearest_full_level_outside():
    """inside: linear in ln p and exact at a full level; above level 0 and below level 7 the level's own value"""
    x = np.arange(8.0).reshape(8, 1, 1) ** 2
    ps = np.full((1, 1), 1.0e5)
    levels = [1.0e5 * ref.FSG[3], 1000.0, 1.0e5, 1.0e5 * np.sqrt(ref.FSG[3] * ref.FSG[4])]
    got = ref.to_levels(x, ps, levels)[:, 0, 0]
    assert abs(got[0] - 9.0) <= 1e-13 and got[1] == 0.0 and got[2] == 49.0 and abs(got[3] - 12.5) <= 1e-12


def _names(*names):
    return (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names]), len(names)


@pytest.mark.parametrize("names, message", [
    (("tcwv", "olr"), b"unknown variable 'olr'"),
    (("t_grid",), b"unknown variable 't_grid'"),
    (("mslp",), b"unknown variable 'mslp'"),
    (("tcwv", "omega_plev", "tcwv"), b"variable 'tcwv' named twice"),
    (("tcwv", "omega_plev"), b"null model"),
])
def test_compute_checks_its_arguments_first(hip_lib, names, message):
    arr, n = _names(*names)
    assert hip_lib.spd_model_derive_compute(None, arr, n, 0, 1, 1, None) == -1
    assert message in hip_lib.spd_last_error(), hip_lib.spd_last_error()
    assert b"spd_model_derive_compute" in hip_lib.spd_last_error()


def test_argument_checks_come_in_the_headers_order(hip_lib):
    """unknown name, name twice, then the null model (a pressure-level name without levels needs a model: the GPU tier has it):
    each case is wrong in everything that comes later as well"""
    cases = [(("olr", "olr"), b"unknown variable"), (("tcwv", "tcwv"), b"named twice"), (("tcwv",), b"null model")]
    for names, message in cases:
        arr, n = _names(*names)
        assert hip_lib.spd_model_derive_compute(None, arr, n, -1, -1, 1, None) == -1
        assert message in hip_lib.spd_last_error(), (names, hip_lib.spd_last_error())
    one = C.create_string_buffer(8)
    for name, dst, message in ((None, one, b"null argument"), (b"tcwv", None, b"null argument"), (b"olr", one, b"unknown variable 'olr'"),
                               (b"tcwv", one, b"null model")):
        assert hip_lib.spd_model_derive_read(None, name, 0, 1, dst, 8, None) == -1
        assert message in hip_lib.spd_last_error(), (name, hip_lib.spd_last_error())


def test_recorders_know_the_names_and_keep_their_messages(hip_lib):
    """the recorders' name check passes the new names (the next complaint is about something else) and an unknown name still gets
    the list it always got, with the derived names behind it"""
    arr, n = _names("omega_plev", "tcwv", "vor_grid")
    assert hip_lib.spd_model_tape_configure(None, arr, n, 4, 3, 1) == -1
    assert b"null model" in hip_lib.spd_last_error(), hip_lib.spd_last_error()
    arr, n = _names("tcwv", "olr")
    assert hip_lib.spd_model_stats_configure(None, arr, n, 4, 0) == -1
    text = hip_lib.spd_last_error()
    assert b"unknown variable 'olr' (u_grid, v_grid, t_grid, q_grid, phi_grid, ps_grid, precnv, precls, u_plev, v_plev, t_plev, " in text
    assert text.endswith(b"q_plev, z_plev, mslp); derived fields: vor_grid, div_grid, omega_grid, rh_grid, theta_grid, tcwv, ivt_u, ivt_v, "
                         b"ke_col, omega_plev, vor_plev, div_plev, rh_plev, theta_plev"), text


NEW_SYMBOLS = ("spd_model_derive_compute", "spd_model_derive_read")


def test_new_symbols_declared_and_exported(hip_lib):
    """The two procedures are declared in include/pyspeedy_amd.h, exported by the built library, bound by ctypes, and have Fortran
    interfaces; the Python layer has the method and the fourteen names."""
    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(spd_[a-z0-9_]+)\s*\(", text))
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name + " is not declared in pyspeedy_amd.h"
        assert hasattr(raw, name), "libpyspeedy_amd.so does not export " + name
        assert name in L.EXPORTED_SYMBOLS
        assert 'bind(C, name="%s")' % name in fortran
    assert hasattr(EnsembleModel, "derived")
    assert EnsembleModel.DERIVED_VARIABLES == ref.NAMES
