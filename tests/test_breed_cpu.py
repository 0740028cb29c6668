"""CPU tier: the breeding norm's definition pinned to the spectra's arbiter through the breeding arbiter
(tests/breed_reference.py) on the golden states; pyspeedy_amd.breed_weights; the argument checks the library makes before anything
is allocated; the entry points (spd_model_breed_*, spd_breed_check) are declared, exported and bound; the example parses its
arguments."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

import breed_reference as ref
import spectra_reference as spectra_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BREED_SYMBOLS = ("spd_breed_check", "spd_model_breed_configure", "spd_model_breed_apply", "spd_model_breed_compute", "spd_model_breed_read",
                 "spd_model_breed_rows", "spd_model_breed_reset", "spd_model_breed_info")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def tables(golden_dir):
    return np.load(os.path.join(golden_dir, "tables.npz"))


# ---- the normalisation -------------------------------------------------------------------------------------------------------
def test_normalisation_is_the_spectra_s(golden_dir, tables):
    """The arbiter's E terms are the spectra of the difference field summed over l: E(vor, k) + E(div, k) = sum_l (ke_rot + ke_div),
    E(t, k) = sum_l t_spectrum, and the same for tr and ps -- which pins w_m, 1/4 and 1/2 (a wrong one shows as a factor 2 or
    sqrt 2).  The two sum the same products in different orders: 527 x 2 non-negative terms per plane, within 1054 x 2^-53 =
    1.2e-13 of each other; bound 1e-12."""
    run = np.load(os.path.join(golden_dir, "run.npz"))
    xp = {n: run["d3_" + n] for n in ref.NAMES}
    xc = {n: run["d1_" + n] for n in ref.NAMES}
    elm2 = tables["elm2"]
    e = ref.energies(xp, xc, elm2)
    d = {n: xp[n][..., 0] - xc[n][..., 0] for n in ref.NAMES}
    s = spectra_ref.spectra(d["vor"], d["div"], d["t"], d["tr"], d["ps"], elm2)
    want = {"ke": (s["ke_rot_spectrum"] + s["ke_div_spectrum"]).sum(axis=-1), "t": s["t_spectrum"].sum(axis=-1),
            "tr": s["q_spectrum"].sum(axis=-1), "ps": np.array([s["lnps_spectrum"].sum()])}
    got = {"ke": e["vor"] + e["div"], "t": e["t"], "tr": e["tr"], "ps": e["ps"]}
    for n in want:
        assert got[n].shape == want[n].shape and (want[n] >= 0).all() and (want[n] > 0).sum() >= len(want[n]) - 2, n
        worst = float((np.abs(got[n] - want[n]) / np.where(want[n] > 0, want[n], 1.0)).max())  # (tr is zero at the top two levels)
        print("E against the spectra, %s: %.2e" % (n, worst))
        assert worst < 1e-12, (n, worst)
    # the amplitude is the square root of the weighted sum of the same numbers
    weights = {n: np.linspace(0.5, 2.0, 8) for n in ref.NAMES}
    a2 = sum(float((weights[n][:len(e[n])] * e[n]).sum()) for n in ref.NAMES)
    assert abs(ref.amplitude(xp, xc, weights, elm2) / math.sqrt(a2) - 1.0) < 1e-12


def test_arbiter_rescale_touches_the_triangle_only():
    rng = np.random.default_rng(0)
    xp = rng.standard_normal((31, 32, 8, 2)) + 1j * rng.standard_normal((31, 32, 8, 2))
    xc = rng.standard_normal((31, 32, 8, 2)) + 1j * rng.standard_normal((31, 32, 8, 2))
    out = ref.rescale_variable(xp, xc, 0.5)
    assert np.array_equal(out[~ref.INSIDE], xp[~ref.INSIDE]) and int(ref.INSIDE.sum()) == 527
    assert np.array_equal(out[ref.INSIDE].real, (xc.real + 0.5 * (xp.real - xc.real))[ref.INSIDE])
    assert np.array_equal(ref.rescale_variable(xp, xp, 3.0), xp)  # (a member equal to its control stays)


# ---- the weights ---------------------------------------------------------------------------------------------------------------
def test_breed_weights_values(tables):
    from pyspeedy_amd import breed_weights
    dhs = tables["dhs"]
    assert dhs.shape == (8,) and abs(dhs.sum() - 1.0) < 1e-7
    zero = np.zeros(8)
    ke = breed_weights("kinetic_energy")
    assert tuple(ke) == ref.NAMES
    assert np.array_equal(ke["vor"], dhs) and np.array_equal(ke["div"], dhs)  # (the model's own table, bit for bit)
    assert all(np.array_equal(ke[n], zero) for n in ("t", "tr", "ps"))
    te = breed_weights("total_energy")
    cp, tref = 1004.0, 270.0
    assert np.array_equal(te["vor"], dhs) and np.array_equal(te["div"], dhs) and np.array_equal(te["tr"], zero)
    assert np.allclose(te["t"], cp / tref * dhs, rtol=1e-15, atol=0.0)
    assert np.isclose(te["ps"][0], 2.0 / 7.0 * cp * tref, rtol=1e-7) and not te["ps"][1:].any()
    trms = breed_weights("t_rms")
    assert np.array_equal(trms["t"], dhs) and all(np.array_equal(trms[n], zero) for n in ("vor", "div", "tr", "ps"))
    some = breed_weights("kinetic_energy", levels=(2, 3))
    assert np.array_equal(some["vor"][2:4], dhs[2:4]) and not some["vor"][:2].any() and not some["vor"][4:].any()
    assert breed_weights()["vor"].tolist() == ke["vor"].tolist()  # (the default kind)
    with pytest.raises(ValueError, match="unknown kind"):
        breed_weights("enstrophy")


def test_python_weight_table():
    from pyspeedy_amd.model import EnsembleModel
    t = EnsembleModel._breed_table({"t": np.arange(8.0), "ps": 3.0})
    assert t.shape == (5, 8) and t[2].tolist() == list(range(8)) and t[4].tolist() == [3.0] + [0.0] * 7 and not t[:2].any()
    with pytest.raises(ValueError, match="unknown variable"):
        EnsembleModel._breed_table({"phi": np.ones(8)})
    with pytest.raises(ValueError, match="shape"):
        EnsembleModel._breed_table({"t": np.ones(7)})


# ---- the argument checks -------------------------------------------------------------------------------------------------------
def _check(hip_lib, control, weights=None, target=1.0, every=4, capacity=8, in_loop=1, null_weights=False):
    """spd_breed_check: what spd_model_breed_configure checks, for len(control) members, without a model"""
    w = np.zeros((5, 8))
    w[0] = 1.0
    for at, value in (weights or {}).items():
        w[at] = value
    ctl = None if control is None else np.asarray(control, dtype=np.int32)
    rc = hip_lib.spd_breed_check(None if ctl is None else ctl.ctypes.data_as(C.POINTER(C.c_int32)), 0 if ctl is None else len(ctl),
                                 None if null_weights else w.ctypes.data_as(C.POINTER(C.c_double)), target, every, capacity, in_loop)
    return rc, hip_lib.spd_last_error()


@pytest.mark.parametrize("control, kwargs, message", [
    ([-1, 0, 1], {}, b"the control of member 2 (1) is itself bred: a control must have -1 (no chains)"),   # a chain of controls
    ([1, 0], {}, b"the control of member 0 (1) is itself bred"),                                          # (two members, each other's)
    ([-1, 1, 0], {}, b"member 1 is its own control"),                                                     # control[i] == i
    ([-1, 0, 3], {}, b"the control of member 2 (3) is out of range (-1 ... 2)"),                          # an index out of range
    ([-1, -2, 0], {}, b"the control of member 1 (-2) is out of range"),
    ([-1, 0, 0], dict(weights={(2, 3): -1e-300}), b"the weight of 't' at level 3 is not a finite number >= 0"),  # a negative weight
    ([-1, 0, 0], dict(weights={(4, 0): NAN}), b"the weight of 'ps' at level 0 is not"),
    ([-1, 0, 0], dict(weights={(1, 7): INF}), b"the weight of 'div' at level 7 is not"),
    ([-1, 0, 0], dict(weights={0: 0.0}), b"all weights are zero"),                         # all weights zero
    ([-1, 0, 0], dict(weights={0: 0.0, (4, 5): 1.0}), b"all weights are zero"),            # (ps reads entry 0 only)
    ([-1, 0, 0], dict(null_weights=True), b"null weights"),
    ([-1, 0, 0], dict(target=0.0), b"target must be a finite number > 0"),                                # target <= 0
    ([-1, 0, 0], dict(target=-1.0), b"target must be"),
    ([-1, 0, 0], dict(target=NAN), b"target must be"),
    ([-1, 0, 0], dict(every=0), b"every must be at least 1"),                                             # every < 1
    ([-1, 0, 0], dict(capacity=0), b"capacity must be at least 1"),
    ([-1, 0, 0], dict(in_loop=2), b"in_loop must be 0 or 1"),
])
def test_a_bad_configuration_is_refused_with_its_message(hip_lib, control, kwargs, message):
    rc, text = _check(hip_lib, control, **kwargs)
    assert rc == -1
    assert message in text, text
    assert b"spd_model_breed_configure" in text


def test_good_configurations_pass_the_checks(hip_lib):
    assert _check(hip_lib, [-1, 0, 0])[0] == 0
    assert _check(hip_lib, [-1, 0, 0, 0, 0, 0, 0, -1])[0] == 0
    assert _check(hip_lib, [-1, -1])[0] == 0  # (no bred member: allowed, launches nothing)
    assert _check(hip_lib, [2, 2, -1], weights={0: 0.0, (4, 0): 1e-300}, target=1e-300, every=1, capacity=1, in_loop=0)[0] == 0


def test_configure_checks_its_arguments_before_it_needs_a_model(hip_lib):
    """spd_model_breed_configure on a null model: everything that does not need the member count is refused first, in the
    documented order; then the null model.  (The controls need the model's member count: spd_breed_check above, and on the device
    tests/test_breed_gpu.py.)"""
    ctl = (C.c_int32 * 3)(-1, 0, 0)

    def configure(w, target, every, capacity, in_loop, control=ctl):
        table = None if w is None else w.ctypes.data_as(C.POINTER(C.c_double))
        rc = hip_lib.spd_model_breed_configure(None, control, table, target, every, capacity, in_loop)
        return rc, hip_lib.spd_last_error()

    good = np.zeros((5, 8))
    good[1, 2] = 1.0
    negative = good.copy()
    negative[3, 4] = -2.0
    # each case is wrong in everything that comes later as well
    cases = [(None, -1.0, 0, 0, 7, b"null weights"),
             (negative, -1.0, 0, 0, 7, b"the weight of 'tr' at level 4"),
             (np.zeros((5, 8)), -1.0, 0, 0, 7, b"all weights are zero"),
             (good, -1.0, 0, 0, 7, b"target must be"),
             (good, 2.0, 0, 0, 7, b"every must be"),
             (good, 2.0, 3, 0, 7, b"capacity must be"),
             (good, 2.0, 3, 5, 7, b"in_loop must be"),
             (good, 2.0, 3, 5, 1, b"spd_model_breed_configure: null model")]
    for w, target, every, capacity, in_loop, message in cases:
        rc, text = configure(w, target, every, capacity, in_loop)
        assert rc == -1 and message in text, (message, text)
    # switching off looks at nothing but the model
    rc, text = configure(None, -1.0, 0, 0, 7, control=None)
    assert rc == -1 and b"spd_model_breed_configure: null model" in text


def test_calls_on_a_null_model_fail_with_a_message(hip_lib):
    rows = (C.c_int32 * 6)()
    n, big = C.c_int(), C.c_longlong()
    assert hip_lib.spd_model_breed_apply(None, None) == -1 and b"spd_model_breed_apply: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_breed_compute(None, None, 0, None) == -1 and b"spd_model_breed_compute: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_breed_read(None, 0, 0, 1, None, 0, None) == -1 and b"spd_model_breed_read: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_breed_read(None, 2, 0, 1, None, 0, None) == -1 and b"what is 0 (amplitude) or 1 (factor)" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_breed_rows(None, rows, 1) == -1 and b"spd_model_breed_rows: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_breed_reset(None) == -1 and b"spd_model_breed_reset: null model" in hip_lib.spd_last_error()
    assert hip_lib.spd_model_breed_info(None, C.byref(n), None, None, C.byref(big), None, None) == -1
    assert b"spd_model_breed_info: null model" in hip_lib.spd_last_error()


# ---- the symbols and the example -------------------------------------------------------------------------------------------------
def test_breed_symbols_declared_exported_and_bound(hip_lib):
    import pyspeedy_amd
    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    header = open(os.path.join(ROOT, "include", "pyspeedy_amd.h")).read()
    fortran = open(os.path.join(ROOT, "include", "pyspeedy_amd_c.f90")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in BREED_SYMBOLS:
        assert name + "(" in header, name
        assert 'bind(C, name="%s")' % name in fortran, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    for method in ("breed_configure", "breed_off", "breed_apply", "breed_amplitude", "breed", "breed_times", "breed_steps", "breed_info",
                   "breed_reset", "breed_growth"):
        assert hasattr(EnsembleModel, method), method
    assert EnsembleModel.BREED_NAMES == ref.NAMES == L.BREED_NAMES
    assert pyspeedy_amd.breed_weights is L.breed_weights and "breed_weights" in pyspeedy_amd.__all__


def test_bred_vectors_example_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("bred_vectors", os.path.join(ROOT, "examples", "bred_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse([])
    assert (args.members, args.days, args.every, args.norm, args.noise) == (8, 10, 9, "kinetic_energy", 0.01)
    args = mod.parse(["--members", "64", "--days", "30", "--every", "36", "--norm", "total_energy", "--noise", "0.1"])
    assert (args.members, args.days, args.every, args.norm, args.noise) == (64, 30, 36, "total_energy", 0.1)
    assert mod.control_of(4).tolist() == [-1, 0, 0, 0]  # (member 0 is the control of all others)
    with pytest.raises(SystemExit):
        mod.parse(["--members", "1"])
    with pytest.raises(SystemExit):
        mod.parse(["--every", "0"])
    with pytest.raises(SystemExit):
        mod.parse(["--norm", "enstrophy"])
