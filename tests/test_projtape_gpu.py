"""GPU tier: weighted sums of the state's grid-space fields recorded on the device as scalar series (spd_model_projtape_*,
EnsembleModel.projtape_*).

The arbiter is existing code: a twin model built by `perturbed` of tests/test_tape_gpu.py (t_grid += N(0, 0.01 K), seed = member id)
that holds an fp64 TAPE of all fourteen names with every = the recorder's.  Each taped plane an entry names is reduced on the CPU by
tests/projtape_reference.py: project, the numpy restatement of the recorder's order that tests/test_projtape_cpu.py holds to a loop
over Python floats.  Every comparison is BITWISE.

A member's trajectory does not depend on how many members its model has or on the launch plan, so one twin of 9 members serves every
fp64 case and one twin of 4 members the fp32-storage case."""
import ctypes as C
from datetime import datetime

import numpy as np
import pytest

import projtape_reference as ref
from test_tape_gpu import LEVELS, perturbed

pytestmark = pytest.mark.gpu

SIGMA8 = ("u_grid", "v_grid", "t_grid", "q_grid", "phi_grid")
ONE = ("ps_grid", "precnv", "precls", "mslp")
PLEV5 = ("u_plev", "v_plev", "t_plev", "q_plev", "z_plev")
NAMES = SIGMA8 + ("ps_grid", "precnv", "precls") + PLEV5 + ("mslp",)  # the catalogue's order
EVERY = 3
CALLS = (5, 1, 7, 12, 3, 20)  # 48 steps and 16 samples, most of them inside calls
TOTAL = sum(CALLS)
SAMPLES = TOTAL // EVERY
STATE = ("vor", "div", "t", "tr", "ps")
STATION = (39.0, -30.0)  # between grid points, where it rains within the 48 steps (convective precipitation is zero at most points)
P = 4  # global mean, a box across the date line, the station, N(0, 1)
RANDOM = 3


def planes_of(name):
    """the first and the last level of a name"""
    return (0,) if name in ONE else (0, 7) if name in SIGMA8 else (0, len(LEVELS) - 1)


# pattern outermost: the entries of one plane lie 24 apart in the list, and the recorder has to find them
ENTRIES = tuple((name, level, p) for p in range(P) for name in NAMES for level in planes_of(name))
assert len(NAMES) == 14 and len(ENTRIES) == 96


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


@pytest.fixture(scope="module")
def weights():
    import pyspeedy_amd
    pw = pyspeedy_amd.projection_weights()
    w = np.stack([pw.global_mean(), pw.box(150.0, -150.0, -40.0, 25.0), pw.point(*STATION),
                  np.random.default_rng(2024).normal(0.0, 1.0, (48, 96))])
    assert w.shape == (P, 48, 96) and (w[RANDOM] < 0).any() and (w[RANDOM] > 0).any() and np.count_nonzero(w[2]) == 4
    return w


def arbiter(spectral, bc, weights, M, fp32=False):
    """dict(planes: {(name, level): numpy [M][16][48][96]} from the twin's fp64 tape, ref: [M][16][E] by projtape_reference, rows,
    state: the spectral state after step 48)"""
    import torch
    model, _ = perturbed(spectral, bc, M, fp32)
    model.tape_configure(NAMES, EVERY, SAMPLES, dtype="float64")
    model.run(TOTAL)
    assert model.tape_info["taken"] == SAMPLES
    wanted = sorted({(n, k) for n, k, _ in ENTRIES})
    planes = {}
    for name in NAMES:
        x = model.tape(name)
        for n, k in wanted:
            if n == name:
                planes[(n, k)] = (x if n in ONE else x[:, :, k]).cpu().numpy()
        del x
    rows = model._tape_rows().tolist()
    torch.cuda.synchronize()
    state = {n: [model.get(n, i) for i in range(M)] for n in STATE}
    model.close()
    out = np.stack([ref.project(weights[p], planes[(n, k)]) for n, k, p in ENTRIES], axis=2)
    assert out.shape == (M, SAMPLES, len(ENTRIES)) and np.isfinite(out).all()
    return dict(planes=planes, ref=out, rows=rows, state=state)


@pytest.fixture(scope="module")
def twin9(spectral, bc, weights):
    return arbiter(spectral, bc, weights, 9)


def assert_bitwise(got, expected, what):
    """got: a device tensor, expected: numpy"""
    got = got.cpu().numpy()
    assert got.shape == expected.shape and got.dtype == expected.dtype, (what, got.shape, expected.shape, got.dtype)
    if not np.array_equal(got, expected):
        bad = got != expected
        where = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d values differ, first at %s (entry %s): %r against %r, max |diff| %.3e" % (
            what, int(bad.sum()), bad.size, where.tolist(), ENTRIES[where[-1]] if bad.shape[-1] == len(ENTRIES) else "?",
            got[tuple(where)], expected[tuple(where)], float(np.abs(got - expected).max())))


# the planes the model itself holds constant over these 48 steps, for every member: specific humidity at the top level, which the
# column physics keeps at zero in the stratosphere, and at 10 hPa, above the top level, which takes the top level's value.  Their
# entries are compared bitwise like all the others; they cannot vary.
CONSTANT_PLANES = {("q_grid", 0), ("q_plev", 4)}


def test_the_arbiter_is_not_empty(twin9, weights):
    """Per entry the series varies over the samples and over the members -- but for the entries of a plane that the taped field
    itself holds constant (CONSTANT_PLANES: asserted to be exactly those whose tape is one value at every point); under the random
    pattern np.sum gives other bits than the stated order somewhere on the arbiter's own data -- a recorder that summed in another
    order would otherwise pass."""
    out = twin9["ref"]
    flat = []
    for e, entry in enumerate(ENTRIES):
        over_samples = (out[:, 1:, e] != out[:, :-1, e]).any()
        over_members = (out[1:, :, e] != out[:-1, :, e]).any()
        print("%-9s level %d pattern %d: %3d distinct values of %d" % (entry + (len(np.unique(out[:, :, e])), out[:, :, e].size)))
        if not (over_samples and over_members):
            flat.append(entry)
    constant = {key for key, x in twin9["planes"].items() if (x == x.flat[0]).all()}
    print("entries that do not vary:", flat, "planes the tape holds constant:", sorted(constant))
    assert constant == CONSTANT_PLANES
    assert sorted(flat) == sorted(e for e in ENTRIES if e[:2] in CONSTANT_PLANES)
    differs = 0
    for (name, level), x in twin9["planes"].items():
        plain = np.sum(weights[RANDOM] * x, axis=(2, 3))
        stated = ref.project(weights[RANDOM], x)
        assert np.allclose(plain, stated, rtol=1e-9, atol=1e-9 * np.abs(weights[RANDOM] * x).sum(axis=(2, 3)).max())
        differs += int((plain != stated).sum())
    print("np.sum differs from the stated order in %d of %d sums under the random pattern" % (differs, 24 * out[:, :, 0].size))
    assert differs > 0


PLANS = {
    "serial_5": dict(M=5),
    "two_groups_5": dict(M=5, options=(("member_groups", 2),)),
    "rounds_9": dict(M=9, options=(("member_groups", 2), ("block_members", 1)), checked=True),
    "fp32_storage_4": dict(M=4, fp32=True),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_series_equal_the_projected_tape(spectral, bc, weights, twin9, plan):
    """All fourteen names at their first and last level under all four patterns, a sample every 3 steps over calls of 5, 1, 7, 12,
    3 and 20 steps: the ring is bitwise the arbiter's, the rows are the tape's, and the recording model's spectral state after step
    48 is bitwise the twin's -- serial, with two uneven member groups, in rounds of block_members with checked calls (the last round
    leaves a group empty), and with fp32 physics storage (precnv / precls stored as float).  With capacity 8 the ring has wrapped
    and holds the last 8."""
    import torch
    p = PLANS[plan]
    M, options, fp32, checked = p["M"], p.get("options", ()), p.get("fp32", False), p.get("checked", False)
    twin = arbiter(spectral, bc, weights, M, fp32=True) if fp32 else twin9
    for capacity in (SAMPLES, 8):
        model, _ = perturbed(spectral, bc, M, fp32, options)
        model.projtape_configure(weights, ENTRIES, EVERY, capacity)
        cfg = model.config()
        if plan == "serial_5":
            assert cfg["chunks"] == 1 and cfg["rounds"] == 1
        if plan == "two_groups_5":
            assert cfg["chunks"] == 2 and cfg["rounds"] == 1
        if plan == "rounds_9":
            assert cfg["chunks"] == 2 and cfg["rounds"] == 5
        if plan == "fp32_storage_4":
            assert cfg["physics_storage32"] and model.device_view("precnv").dtype == torch.float32
        assert model.projtape_entries == ENTRIES
        for n in CALLS:
            if checked:
                failed, _ = model.run_checked(n)
                assert (failed == -1).all()
            else:
                model.run(n)
        assert model.current_step == TOTAL
        held = min(capacity, SAMPLES)
        assert model.projtape_info == dict(taken=SAMPLES, held=held, capacity=capacity, every=EVERY, patterns=P, entries=len(ENTRIES))
        assert model._projtape_rows().tolist() == twin["rows"][SAMPLES - held:]
        assert model.projtape_steps().tolist() == list(range(EVERY * (SAMPLES - held + 1), TOTAL + 1, EVERY))
        assert_bitwise(model.projtape(), twin["ref"][:M, SAMPLES - held:], "%s, capacity %d" % (plan, capacity))
        for n, per_member in twin["state"].items():
            for i in range(M):
                assert np.array_equal(model.get(n, i), per_member[i]), (plan, capacity, n, i)
        model.close()


LIFE = (("t_grid", 7, 0), ("z_plev", 4, 2), ("precls", 0, RANDOM), ("t_grid", 7, RANDOM), ("mslp", 0, 1))
LIFE_COLUMNS = [ENTRIES.index(e) for e in LIFE]


def test_configured_after_two_steps_reset_sub_ranges_and_off(spectral, bc, weights, twin9):
    """A recorder configured at step 2 takes its first sample at step 3; _reset empties the ring; reads of sub-ranges of members and
    samples give the matching slices; a reconfiguration replaces entries and patterns; n_entries = 0 switches off, after which
    calls fail with their reason; reconfiguring the pressure levels is refused while a pressure-level entry exists."""
    import torch
    from pyspeedy_amd._lib import SpeedyHipError
    M = 3
    expected = twin9["ref"][:M][:, :, LIFE_COLUMNS]
    model, _ = perturbed(spectral, bc, M)
    with pytest.raises(SpeedyHipError, match="no projection tape configured"):
        model.projtape_info
    assert model.projtape_entries == ()
    model.run(2)
    model.projtape_configure(weights, LIFE, EVERY, 6)
    assert model.projtape_info == dict(taken=0, held=0, capacity=6, every=EVERY, patterns=P, entries=len(LIFE))
    assert model.projtape().shape == (M, 0, len(LIFE)) and model.projtape_steps().tolist() == []
    for n in (3, 1, 7, 2):  # to step 15
        model.run(n)
    assert model.projtape_steps().tolist() == [3, 6, 9, 12, 15]
    assert model.projtape_times()[:2] == [datetime(1982, 1, 1, 2, 0), datetime(1982, 1, 1, 4, 0)]
    whole = model.projtape()
    assert_bitwise(whole, expected[:, 0:5], "configured at step 2")
    assert_bitwise(model.projtape(first=1, count=2, t0=1, nt=3), expected[1:3, 1:4], "members 1, 2 and samples 1 ... 3")
    assert_bitwise(model.projtape(first=2, t0=4), expected[2:3, 4:5], "member 2, the last sample")
    assert_bitwise(torch.cat([model.projtape(t0=0, nt=2), model.projtape(t0=2, nt=3)], dim=1), expected[:, 0:5], "in two parts")
    one = np.zeros((1, 6), dtype=np.int32)
    assert model._lib.spd_model_projtape_times(model._m, one.ctypes.data_as(C.POINTER(C.c_int32)), 1) == 1  # (the oldest held)
    assert one.tolist() == [[3, 1982, 1, 1, 2, 0]]
    buf = torch.empty(4, dtype=torch.float64, device=model.sp.device)
    assert model._lib.spd_model_projtape_read(model._m, 0, M, 0, 5, buf.data_ptr(), 32, None) == -3  # SPD_E_SIZE
    with pytest.raises(SpeedyHipError, match="sample range out of bounds"):
        model.projtape(t0=3, nt=3)
    with pytest.raises(SpeedyHipError, match="member range out of bounds"):
        model.projtape(first=2, count=2)
    model.projtape_reset()  # at step 15
    assert model.projtape_info["taken"] == 0 and model.projtape().shape == (M, 0, len(LIFE))
    model.run(9)
    assert model.projtape_steps().tolist() == [18, 21, 24]
    assert_bitwise(model.projtape(), expected[:, 5:8], "after the reset")
    with pytest.raises(SpeedyHipError, match="the projection tape holds a pressure-level variable"):
        model.plev_configure([500.0])
    # other entries, two patterns in another order, another rhythm: at step 24
    second = (("q_grid", 0, 1), ("precnv", 0, 0), ("q_grid", 0, 0))
    model.projtape_configure(weights[[RANDOM, 0]], second, 6, 4)
    assert model.projtape_entries == second and model.projtape_info["patterns"] == 2 and model.projtape_info["taken"] == 0
    model.run(12)
    assert model.projtape_steps().tolist() == [30, 36]
    columns = [ENTRIES.index(e) for e in (("q_grid", 0, 0), ("precnv", 0, RANDOM), ("q_grid", 0, RANDOM))]
    assert_bitwise(model.projtape(), twin9["ref"][:M][:, [9, 11]][:, :, columns], "reconfigured")
    # a refused configuration leaves the recorder as it was when the refusal comes before a model is needed ...
    with pytest.raises(SpeedyHipError, match="pattern 2 of entry 0"):
        model.projtape_configure(weights[:2], [("t_grid", 0, 2)], 3, 4)
    assert model.projtape_entries == second and model.projtape_info["taken"] == 2
    with pytest.raises(ValueError, match=r"weights must be \[P\]\[48\]\[96\]"):
        model.projtape_configure(weights[0], second, 3, 4)
    with pytest.raises(ValueError, match="an entry is"):
        model.projtape_configure(weights, [("t_grid", 0)], 3, 4)
    # ... a pressure-level level beyond the configured count is found with the model, before the recorder goes
    with pytest.raises(SpeedyHipError, match=r"level 5 of entry 0 \('z_plev'\) is out of range \(0 ... 4\)"):
        model.projtape_configure(weights, [("z_plev", 5, 0)], 3, 4)
    assert model.projtape_info["taken"] == 2
    # off
    model.projtape_configure([], [], 0, 0)
    assert model.projtape_entries == ()
    for call in (model.projtape, model.projtape_reset, model.projtape_steps, lambda: model.projtape_info):
        with pytest.raises(SpeedyHipError, match="no projection tape configured"):
            call()
    model.plev_configure([500.0])
    model.run(3)
    model.close()


def test_checked_calls_validity_and_init(spectral, bc, weights):
    """Configuration, reset and reads are refused while a checked call is in flight; a checked call that reports a failed range
    check (the model's own check, on a member whose temperature was set out of range) makes reads fail, naming member and step,
    until the next reset; spd_model_init empties the ring."""
    from pyspeedy_amd._lib import SpeedyHipError
    M = 2
    entries = (("ps_grid", 0, 0), ("t_grid", 7, 2))
    model, _ = perturbed(spectral, bc, M)
    model.projtape_configure(weights, entries, 3, 4)
    stream = model._stream()
    assert model._lib.spd_model_step_checked_begin(model._m, 4, stream) == 0
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.projtape()
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.projtape_configure(weights, entries, 3, 4)
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.projtape_reset()
    failed = np.zeros(M, dtype=np.int32)
    assert model._lib.spd_model_step_checked_end(model._m, failed.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    assert failed.tolist() == [-1, -1] and model.projtape_steps().tolist() == [3]
    assert model.projtape_entries == entries
    # a member out of range: global-mean temperature of 500 K (diagnostics.f90:57-66), as tests/test_tape_gpu.py
    t = model.get("t", 1)
    t[0, 0, :, :] = 500.0 * np.sqrt(2.0)
    model.set("t", t, member=1)
    failed, _ = model.run_checked(3)
    assert failed.tolist() == [-1, 0]
    with pytest.raises(SpeedyHipError, match="invalid until spd_model_projtape_reset: member 1 failed the range check at step 0"):
        model.projtape()
    assert model.projtape_info["taken"] == 2  # (the count is still told)
    model.projtape_reset()
    assert model.projtape().shape == (M, 0, 2)
    # spd_model_init: an empty ring, the configuration stays
    model.init((1982, 1, 1, 0, 0))
    model.run(7)
    assert model.projtape_steps().tolist() == [3, 6]
    model.init((1982, 1, 1, 0, 0))
    assert model.projtape_info == dict(taken=0, held=0, capacity=4, every=3, patterns=P, entries=2)
    model.close()


def test_all_seven_recorders_together_in_rounds_with_rings_that_wrap(spectral, bc, weights):
    """Statistics, tape, spectra, ensemble tape, accumulation tape, window tape and projection tape on at once, in ONE checked call
    of 13 steps issued as five rounds (9 members, two member groups, block_members 1: the last round leaves a group empty), into
    rings of two slots that wrap inside the call.  Everything a recorder hands out equals what it hands out when it is the only one
    on in the same plan, and the final state, every registry variable, is bitwise that of a run with none."""
    import torch
    M, steps = 9, 13
    fields = ("t_grid", "precnv")
    names = ("ke_rot_spectrum", "lnps_mean")
    acc = (("precnv", "sum"), ("olr", "mean"))
    win = (("t_grid", "mean"), ("precnv", "max"), ("wspd_grid", "max"))
    proj = (("t_grid", 7, RANDOM), ("precnv", 0, 0), ("t_grid", 7, 0), ("ps_grid", 0, 2), ("u_grid", 3, 1))
    configure = {
        "stats": lambda m: m.stats_configure(fields, 2, variance=True),
        "tape": lambda m: m.tape_configure(fields, 3, 2, dtype="float64"),
        "spectra": lambda m: m.spectra_configure(names, 2, 2),
        "enstape": lambda m: m.enstape_configure(fields, 2, 2),
        "acctape": lambda m: m.acctape_configure(acc, 3, 2, dtype="float64"),
        "wintape": lambda m: m.wintape_configure(win, 2, 2, sample_every=1, dtype="float64"),
        "projtape": lambda m: m.projtape_configure(weights, proj, 2, 2),
    }
    read = {
        "stats": lambda m: dict(samples=m.stats_samples, mean={n: m.stats_mean(n) for n in fields}, var={n: m.stats_var(n) for n in fields}),
        "tape": lambda m: dict(info=m.tape_info, steps=m.tape_steps().tolist(), times=m.tape_times(), data={n: m.tape(n) for n in fields}),
        "spectra": lambda m: dict(info=m.spectra_info(), steps=m.spectra_steps().tolist(), times=m.spectra_times(),
                                  data={n: m.spectra(n) for n in names}),
        "enstape": lambda m: dict(info=m.enstape_info, steps=m.enstape_steps().tolist(), times=m.enstape_times(),
                                  data={n: m.enstape(n) + m.enstape_moments(n)[2:] for n in fields}),
        "acctape": lambda m: dict(info=m.acctape_info, steps=m.acctape_steps().tolist(), times=m.acctape_times(),
                                  counts=m.acctape_counts().tolist(), data={e: m.acctape(*e) for e in acc}),
        "wintape": lambda m: dict(info=m.wintape_info, steps=m.wintape_steps().tolist(), times=m.wintape_times(),
                                  counts=[c.tolist() for c in m.wintape_counts()], data={e: m.wintape(*e) for e in win}),
        "projtape": lambda m: dict(info=m.projtape_info, steps=m.projtape_steps().tolist(), times=m.projtape_times(), data=m.projtape()),
    }
    taken = {"tape": 4, "spectra": 6, "enstape": 6, "acctape": 4, "wintape": 6, "projtape": 6}  # 13 steps from step 0, every 3 or 2

    def run(on):
        model, _ = perturbed(spectral, bc, M, options=(("member_groups", 2), ("block_members", 1)), levels=None)
        assert model.config()["chunks"] == 2 and model.config()["rounds"] == 5
        for key in on:
            configure[key](model)
        failed, _ = model.run_checked(steps)
        assert (failed == -1).all()
        out = {key: read[key](model) for key in on}
        out["state"] = {n: [model.get(n, i) for i in range(M)] for n in model.variables() if n not in ("lon", "lat", "lev")}
        torch.cuda.synchronize()
        model.close()
        return out

    def assert_same(got, expected, what):
        if torch.is_tensor(expected):
            assert got.shape == expected.shape and got.dtype == expected.dtype and torch.equal(got, expected), what
        elif isinstance(expected, dict):
            assert got.keys() == expected.keys(), what
            for k in expected:
                assert_same(got[k], expected[k], "%s, %s" % (what, k))
        elif isinstance(expected, tuple):
            assert len(got) == len(expected), what
            for k, (a, b) in enumerate(zip(got, expected)):
                assert_same(a, b, "%s, %d" % (what, k))
        else:
            assert got == expected, (what, got, expected)

    together, none = run(tuple(configure)), run(())
    assert together["stats"]["samples"] == 6
    for key, n in taken.items():  # (every ring has wrapped)
        assert together[key]["info"]["taken"] == n and together[key]["info"]["held"] == 2 and len(together[key]["steps"]) == 2, key
    assert together["projtape"]["steps"] == [10, 12]
    for key in configure:
        assert_same(together[key], run((key,))[key], key + " beside the others")
    # ... and what the projection tape holds is the projection of what the tape beside it holds at the sample both took (step 12)
    assert together["tape"]["steps"] == [9, 12]
    t_low = together["tape"]["data"]["t_grid"][:, 1, 7].cpu().numpy()
    precnv = together["tape"]["data"]["precnv"][:, 1].cpu().numpy()
    got = together["projtape"]["data"][:, 1].cpu().numpy()
    assert np.array_equal(got[:, 0], ref.project(weights[RANDOM], t_low)) and np.array_equal(got[:, 2], ref.project(weights[0], t_low))
    assert np.array_equal(got[:, 1], ref.project(weights[0], precnv))
    for n, per_member in none["state"].items():
        for i, (a, b) in enumerate(zip(together["state"][n], per_member)):
            assert np.array_equal(a, b), (n, i)


def test_shapes_dtype_device_and_levels(spectral, bc, weights):
    """projtape() is float64 [count][nt][E], contiguous, on the model's device; pressure-level names are refused before levels are
    configured; 64 patterns and a plane under all of them."""
    import torch
    from pyspeedy_amd._lib import SpeedyHipError
    M = 2
    model, views = perturbed(spectral, bc, M, levels=None)
    for name in PLEV5 + ("mslp",):
        with pytest.raises(SpeedyHipError, match="'%s' needs target levels" % name):
            model.projtape_configure(weights, [("t_grid", 0, 0), (name, 0, 0)], 4, 2)
    with pytest.raises(SpeedyHipError, match="no projection tape configured"):
        model.projtape_info
    model.plev_configure([850.0, 500.0, 250.0])
    many = np.random.default_rng(7).normal(0.0, 1.0, (64, 48, 96))
    entries = [("t_grid", 7, p) for p in range(64)] + [("z_plev", 2, 5), ("mslp", 0, 63), ("precls", 0, 0)]
    model.projtape_configure(many, entries, 2, 3)
    model.tape_configure(["t_grid"], 2, 3, dtype="float64")
    model.run(4)
    got = model.projtape()
    assert got.shape == (M, 2, 67) and got.dtype == torch.float64 and got.device == views["t_grid"].device
    assert got.is_contiguous() and bool(torch.isfinite(got).all())
    assert model.projtape(first=1, t0=1).shape == (1, 1, 67) and model.projtape(count=0).shape == (0, 2, 67)
    t_low = model.tape("t_grid")[:, :, 7].cpu().numpy()
    expected = np.stack([ref.project(many[p], t_low) for p in range(64)], axis=2)
    assert np.array_equal(got[:, :, :64].cpu().numpy(), expected)  # (sixteen batches of four entries on one plane)
    model.close()


# an interleaved list that comes back to planes it has left (t_grid 7, z_plev 1 and precnv twice or three times, not adjacent) and
# mixes sigma-level, pressure-level, mslp and precipitation names
MIXED = (("t_grid", 7, 0), ("z_plev", 1, 1), ("precnv", 0, 0), ("t_grid", 7, RANDOM), ("mslp", 0, 1), ("z_plev", 1, 0), ("u_grid", 0, RANDOM),
         ("precnv", 0, 1), ("t_grid", 7, 1))


def by_plane(entries):
    """the order that puts the entries of one plane next to each other: planes as they first appear, the list's order within one"""
    planes = [e[:2] for e in entries]
    return sorted(range(len(entries)), key=lambda k: planes.index(planes[k]))


def test_an_entry_is_a_function_of_its_own_plane_and_pattern(spectral, bc, weights):
    """The sample of step 4 under MIXED, and on a twin brought to the same step under the same entries with equal planes adjacent:
    entry for entry the same bits, for every member.  Holds the table of distinct planes (csrc/entry_front.hpp) to the order of
    the caller's list."""
    order = by_plane(MIXED)
    assert order != list(range(len(MIXED))) and sorted(order) == list(range(len(MIXED)))
    got = []
    for entries in (MIXED, [MIXED[k] for k in order]):
        model, _ = perturbed(spectral, bc, 4, levels=[850.0, 500.0])
        model.run(3)
        model.projtape_configure(weights, entries, 4, 1)
        model.run(1)  # (a one-step call that ends on a sample)
        assert model.projtape_steps().tolist() == [4]
        got.append(model.projtape().cpu().numpy()[:, 0])  # [members][E]
        model.close()
    mixed, sorted_ = got
    assert mixed.shape == (4, len(MIXED)) and np.isfinite(mixed).all()
    assert np.array_equal(mixed[:, order].view(np.uint64), sorted_.view(np.uint64)), np.argwhere(mixed[:, order] != sorted_).tolist()
    assert len(np.unique(mixed[:, [0, 1, 3, 4, 5, 6, 8]])) == 4 * 7  # (the planes but precnv: no two entries or members agree)
