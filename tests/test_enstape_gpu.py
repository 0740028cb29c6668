"""GPU tier: the ensemble mean and spread recorded on the device inside multi-step calls (spd_model_enstape_*,
EnsembleModel.enstape_*).

The arbiter is an fp64 tape on a twin model built by the recipe of tests/test_tape_gpu.py (t_grid += N(0, 0.01 K), seed = member
id), which that file pins bitwise to the hand-rolled loop: x = twin.tape(name) holds every member's value at every sample, and the
ensemble tape must give its mean and unbiased variance over the members within the textbook error bounds of Welford's and Chan's
updates, N eps kappa with kappa = sqrt(1 + mu^2 / sigma^2), in pointwise form and with a factor 4 for the reference's own rounding
and the unit conversion (eps = 2^-52, M members):

    |mean - x.mean(0)| <= 4 M eps max_j |x_j|
    |std^2 - v_ref|    <= 16 M eps (v_ref + |x.mean(0)| sqrt(v_ref)),   v_ref = x.var(0, unbiased=True)

and std^2 == 0 exactly wherever all members hold the same value.  every = 3, calls of (7, 5) steps, capacity 3: four samples are
taken, three are held, slot 0 is used again on the second lap and one sample falls at the end of a call."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("t_grid", "ps_grid", "precnv", "z_plev", "mslp")  # transformed planes, exp() in the unit, stored precision, pressure levels
LEVELS = [500.0, 1000.0]  # hPa
EVERY, CALLS, CAPACITY = 3, (7, 5), 3
STATE = ("vor", "div", "t", "tr", "ps")
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


def perturbed(spectral, bc, M, fp32=False, options=(), levels=LEVELS, noise=True, first_seed=0):
    """tests/test_tape_gpu.py's recipe: t_grid += N(0, 0.01 K) with seed = member id (here: first_seed + member)"""
    import torch
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, M)
    model.set_bc(bc, start_date=(1982, 1, 1, 0, 0))
    for name, value in options:
        model.set_option(name, value)
    if fp32:
        model.set_physics_precision(True)
    if noise:
        model.spectral2grid()
        t_grid = model.device_view("t_grid")
        field = np.stack([np.random.default_rng(first_seed + i).normal(0.0, 0.01, (96, 48, 8)).transpose(2, 1, 0) for i in range(M)])
        t_grid += torch.from_numpy(np.ascontiguousarray(field)).to(t_grid.device)
        model.grid2spectral()
    if levels:
        model.plev_configure(levels)
    return model


def step(model, n, checked=False):
    if checked:
        failed, _ = model.run_checked(n)
        assert (failed == -1).all()
    else:
        model.run(n)


def state_of(model):
    return {n: [model.get(n, i) for i in range(model.nmembers)] for n in STATE}


def moments_of(model, names=NAMES):
    """{name: (mean, std, m2)} of everything the ring holds"""
    out = {}
    for n in names:
        mean, std = model.enstape(n)
        members, mean2, m2 = model.enstape_moments(n)
        assert members == model.nmembers
        assert_bitwise(mean2, mean, "mean of enstape_moments, " + n)
        out[n] = (mean, std, m2)
    return out


def assert_bitwise(got, ref, what):
    import torch
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if not torch.equal(got, ref):
        bad = got != ref
        raise AssertionError("%s: %d of %d values differ, max |diff| %.3e" % (
            what, int(bad.sum()), bad.numel(), float((got.double() - ref.double()).abs().max())))


def assert_within_bounds(mean, std, x, what):
    """mean, std: [nt]...; x: [M][nt]... fp64, the members' values"""
    import torch
    M = x.shape[0]
    assert mean.shape == x.shape[1:] and std.shape == x.shape[1:] and mean.dtype == torch.float64 and std.dtype == torch.float64, what
    ref_mean, v_ref = x.mean(0), x.var(0, unbiased=True)
    err = (mean - ref_mean).abs()
    bound = 4 * M * EPS * x.abs().amax(0)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: mean error / bound %.3f" % (what, worst))
    assert bool((err <= bound).all()), "%s: mean off by %.3f of its bound" % (what, worst)
    v = std * std
    err = (v - v_ref).abs()
    bound = 16 * M * EPS * (v_ref + ref_mean.abs() * v_ref.sqrt())
    worst = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    print("%s: variance error / bound %.3f" % (what, worst))
    assert bool((err <= bound).all()), "%s: variance off by %.3f of its bound" % (what, worst)
    same = (x == x[0:1]).all(0)
    assert bool((v[same] == 0.0).all()), "%s: a spread where all members hold the same value" % what
    return same


PLANS = {
    "serial_8": dict(M=8),
    "groups_25": dict(M=25),
    "rounds_32": dict(M=32, options=(("block_members", 4),), checked=True),
    "fp32_physics_8": dict(M=8, fp32=True),
    "one_step_calls_8": dict(M=8, calls=(1,) * 12),
}
_RUNS = {}


def run_plan(spectral, bc, plan):
    """The recording model and its twin with an fp64 tape, through the plan's calls: everything the tests compare (once per plan)"""
    import torch
    if plan in _RUNS:
        return _RUNS[plan]
    p = PLANS[plan]
    M, options, fp32, checked, calls = p["M"], p.get("options", ()), p.get("fp32", False), p.get("checked", False), p.get("calls", CALLS)
    out = {}
    twin = perturbed(spectral, bc, M, fp32, options)
    twin.tape_configure(NAMES, EVERY, CAPACITY, dtype="float64")
    for n in calls:
        step(twin, n, checked)
    out["x"] = {n: twin.tape(n).clone() for n in NAMES}
    out["twin_steps"], out["twin_times"], out["twin_state"] = twin.tape_steps().tolist(), twin.tape_times(), state_of(twin)
    twin.close()
    model = perturbed(spectral, bc, M, fp32, options)
    model.enstape_configure(NAMES, EVERY, CAPACITY)
    out["config"] = model.config()
    for n in calls:
        step(model, n, checked)
    assert model.current_step == sum(calls)
    out["info"], out["steps"], out["times"] = model.enstape_info, model.enstape_steps().tolist(), model.enstape_times()
    out["moments"] = moments_of(model)
    out["state"] = state_of(model)
    torch.cuda.synchronize()
    model.close()
    _RUNS[plan] = out
    return out


@pytest.mark.parametrize("plan", list(PLANS))
def test_mean_and_spread_equal_the_members_on_an_fp64_tape(spectral, bc, plan):
    """Five names in five launch plans: one group; three uneven groups (25 members); rounds of block_members in checked calls, which
    fold into partials that already hold members; fp32 physics storage (precnv read as fp32); calls of one step."""
    import torch
    r = run_plan(spectral, bc, plan)
    M, cfg = PLANS[plan]["M"], r["config"]
    if plan == "groups_25":
        assert cfg["chunks"] == 3
    if plan == "rounds_32":
        assert cfg["rounds"] > 1
    if plan == "fp32_physics_8":
        assert cfg["physics_storage32"]
    assert r["steps"] == r["twin_steps"] == [6, 9, 12] and r["times"] == r["twin_times"]
    assert r["info"] == dict(taken=4, held=3, capacity=CAPACITY, every=EVERY, members=M)
    for n in NAMES:
        mean, std, m2 = r["moments"][n]
        x = r["x"][n]
        assert x.shape[0] == M and x.shape[1] == 3 and x.dtype == torch.float64
        same = assert_within_bounds(mean, std, x, "%s %s" % (plan, n))
        # enstape_moments agrees with enstape: the standard deviation is sqrt(M2 / (M - 1)), correctly rounded
        assert np.array_equal(std.cpu().numpy(), np.sqrt(m2.cpu().numpy() / (M - 1))), (plan, n)
        assert bool((m2 >= 0).all()) and bool((m2[same] == 0.0).all()), (plan, n)
    # not vacuous: the members differ at more than half of the points of every held sample
    positive = (r["x"]["t_grid"].var(0) > 0).flatten(1).double().mean(1)
    assert bool((positive > 0.5).all()), positive.tolist()
    # recording changes nothing of the run
    for n in STATE:
        for i in range(M):
            assert np.array_equal(r["state"][n][i], r["twin_state"][n][i]), (plan, n, i)


def test_unperturbed_ensemble_has_no_spread(spectral, bc):
    """25 identical members in three groups, with an fp64 tape beside the ensemble tape: the mean is bitwise member 0's value on
    the tape and M2 exactly 0 at every point and sample -- a stale partial, a wrong count of members already folded or a lap that
    did not overwrite its slot would show here."""
    import torch
    model = perturbed(spectral, bc, 25, noise=False)
    model.tape_configure(NAMES, EVERY, CAPACITY, dtype="float64")
    model.enstape_configure(NAMES, EVERY, CAPACITY)
    assert model.config()["chunks"] == 3
    for n in CALLS:
        model.run(n)
    assert model.enstape_info["taken"] == 4 and model.enstape_steps().tolist() == model.tape_steps().tolist() == [6, 9, 12]
    for n in NAMES:
        x = model.tape(n)
        assert_bitwise(x[24], x[0], "the members are identical, " + n)
        members, mean, m2 = model.enstape_moments(n)
        assert members == 25
        assert_bitwise(mean, x[0], "mean of identical members, " + n)
        assert bool((m2 == 0.0).all()), n
        assert bool((model.enstape(n)[1] == 0.0).all()), n
    assert not torch.equal(model.enstape("t_grid")[0][0], model.enstape("t_grid")[0][2])
    model.close()


def test_a_plan_repeats_bit_for_bit(spectral, bc):
    """The 25-member run again: the same launch plan gives the same bits of mean and M2."""
    first = run_plan(spectral, bc, "groups_25")["moments"]
    model = perturbed(spectral, bc, 25)
    model.enstape_configure(NAMES, EVERY, CAPACITY)
    for n in CALLS:
        model.run(n)
    again = moments_of(model)
    model.close()
    for n in NAMES:
        assert_bitwise(again[n][0], first[n][0], "mean of " + n)
        assert_bitwise(again[n][2], first[n][2], "M2 of " + n)


def test_one_member(spectral, bc):
    """A model of one member: the mean is bitwise its fp64 tape, M2 is 0 and the standard deviation NaN."""
    import torch
    model = perturbed(spectral, bc, 1)
    model.tape_configure(NAMES, EVERY, CAPACITY, dtype="float64")
    model.enstape_configure(NAMES, EVERY, CAPACITY)
    for n in CALLS:
        model.run(n)
    for n in NAMES:
        mean, std = model.enstape(n)
        assert_bitwise(mean, model.tape(n)[0], n)
        assert bool(torch.isnan(std).all()), n
        assert bool((model.enstape_moments(n)[2] == 0.0).all()), n
    assert model.enstape_info["members"] == 1
    model.close()


def test_the_four_recorders_are_independent(spectral, bc):
    """Statistics, tape, spectra and ensemble tape on one model, each with its own `every`: the ensemble tape's mean and M2 are
    bitwise what they are with the other three off."""
    alone = run_plan(spectral, bc, "serial_8")["moments"]
    model = perturbed(spectral, bc, 8)
    model.stats_configure(("u_grid", "t_grid", "precnv", "z_plev"), 4, variance=True)
    model.tape_configure(("v_grid", "precnv", "precls", "t_plev", "mslp"), 2, 6, dtype="float32")
    model.spectra_configure(("ke_rot_spectrum", "t_mean"), 5, 2)
    model.enstape_configure(NAMES, EVERY, CAPACITY)
    for n in CALLS:
        model.run(n)
    assert model.stats_samples == 3 and model.tape_info["taken"] == 6 and model.spectra_info()["taken"] == 2
    assert model.enstape_info["taken"] == 4
    together = moments_of(model)
    model.close()
    for n in NAMES:
        assert_bitwise(together[n][0], alone[n][0], "mean of " + n)
        assert_bitwise(together[n][2], alone[n][2], "M2 of " + n)


def test_the_ring(spectral, bc):
    """Sub-ranges of the held samples equal slices of the whole read; after a reset nothing is held and the next sample is the
    first again, in slot 0, where it replaces what the slot held."""
    import torch
    whole = run_plan(spectral, bc, "serial_8")["moments"]
    model = perturbed(spectral, bc, 8)
    model.enstape_configure(NAMES, EVERY, CAPACITY)
    for n in CALLS:
        model.run(n)
    for n in NAMES:
        mean, std = model.enstape(n)
        assert_bitwise(mean, whole[n][0], n)
        for t0, nt in ((0, 1), (1, 2), (2, 1), (0, 3), (3, 0)):
            part_mean, part_std = model.enstape(n, t0=t0, nt=nt)
            assert_bitwise(part_mean, mean[t0:t0 + nt], "%s mean [%d, %d)" % (n, t0, t0 + nt))
            assert_bitwise(part_std, std[t0:t0 + nt], "%s std [%d, %d)" % (n, t0, t0 + nt))
            assert_bitwise(model.enstape_moments(n, t0=t0, nt=nt)[2], whole[n][2][t0:t0 + nt], "%s M2 [%d, %d)" % (n, t0, t0 + nt))
    model.enstape_reset()
    info = model.enstape_info
    assert (info["taken"], info["held"]) == (0, 0) and model.enstape_steps().tolist() == [] and model.enstape_times() == []
    assert model.enstape("mslp")[0].shape == (0, 48, 96)
    model.tape_configure(NAMES, EVERY, 1, dtype="float64")
    model.run(4)  # steps 13 ... 16: one sample, at 15
    info = model.enstape_info
    assert (info["taken"], info["held"]) == (1, 1) and model.enstape_steps().tolist() == model.tape_steps().tolist() == [15]
    for n in NAMES:
        mean, std = model.enstape(n)
        assert_within_bounds(mean, std, model.tape(n), "after the reset, " + n)
    assert not torch.equal(model.enstape("t_grid")[0][0], whole["t_grid"][0][0])
    model.close()


def test_a_lap_inside_one_call_in_rounds(spectral, bc):
    """Capacity 1 and two samples in ONE checked call that runs in rounds: both go to slot 0, and the members of the later rounds
    must not fold their first sample into the partials of the second."""
    options = (("block_members", 4),)
    twin = perturbed(spectral, bc, 32, options=options)
    twin.tape_configure(NAMES, EVERY, 1, dtype="float64")
    step(twin, 7, checked=True)
    model = perturbed(spectral, bc, 32, options=options)
    model.enstape_configure(NAMES, EVERY, 1)
    assert model.config()["rounds"] > 1
    step(model, 7, checked=True)
    assert model.enstape_info == dict(taken=2, held=1, capacity=1, every=EVERY, members=32)
    assert model.enstape_steps().tolist() == twin.tape_steps().tolist() == [6]
    for n in NAMES:
        mean, std = model.enstape(n)
        assert_within_bounds(mean, std, twin.tape(n), "rounds, capacity 1, " + n)
    twin.close()
    model.close()


def test_merge_moments_of_two_models(spectral, bc):
    """Two models of 5 and 3 members with the seeds of the 8-member model: their moments, merged, agree with that model's ensemble
    tape within the bounds."""
    from pyspeedy_amd.ensemble import merge_moments
    whole = run_plan(spectral, bc, "serial_8")
    parts = {n: [] for n in NAMES}
    for first_seed, M in ((0, 5), (5, 3)):
        model = perturbed(spectral, bc, M, first_seed=first_seed)
        model.enstape_configure(NAMES, EVERY, CAPACITY)
        for n in CALLS:
            model.run(n)
        for n in NAMES:
            parts[n].append(model.enstape_moments(n))
        model.close()
    for n in NAMES:
        assert [p[0] for p in parts[n]] == [5, 3]
        members, mean, std = merge_moments(parts[n])
        assert members == 8
        assert_within_bounds(mean, std, whole["x"][n], "merged, " + n)
        x = whole["x"][n]
        mean8, std8, _ = whole["moments"][n]
        v_ref = x.var(0, unbiased=True)
        assert bool(((mean - mean8).abs() <= 4 * 8 * EPS * x.abs().amax(0)).all()), n
        assert bool(((std * std - std8 * std8).abs() <= 16 * 8 * EPS * (v_ref + x.mean(0).abs() * v_ref.sqrt())).all()), n


def test_lifecycle(spectral, bc):
    """Reads before configuring and of unconfigured names fail; a pressure-level name needs levels, and the levels stay while one
    is held; reads are refused while a checked call is in flight and after one that reported a failed range check, naming member
    and step, until the next reset; a short destination is SPD_E_SIZE; an empty list switches the ring off."""
    import torch
    from pyspeedy_amd._lib import SpeedyHipError
    model = perturbed(spectral, bc, 2, levels=None)
    with pytest.raises(SpeedyHipError, match="no ensemble tape configured"):
        model.enstape_info
    with pytest.raises(SpeedyHipError, match="no ensemble tape configured"):
        model.enstape_reset()
    with pytest.raises(SpeedyHipError, match="no ensemble tape configured"):
        model.enstape("t_grid")
    with pytest.raises(SpeedyHipError, match="unknown variable"):
        model.enstape_configure(["t_grid", "olr"], EVERY, 4)
    with pytest.raises(SpeedyHipError, match="every"):
        model.enstape_configure(["t_grid"], 0, 4)
    with pytest.raises(SpeedyHipError, match="capacity"):
        model.enstape_configure(["t_grid"], EVERY, 0)
    with pytest.raises(SpeedyHipError, match="needs target levels"):
        model.enstape_configure(["t_grid", "z_plev"], EVERY, 4)
    model.plev_configure([500.0])
    model.enstape_configure(["t_grid", "z_plev"], EVERY, 4)
    assert model.enstape_info == dict(taken=0, held=0, capacity=4, every=EVERY, members=2)
    assert model.enstape("t_grid")[0].shape == (0, 8, 48, 96) and model.enstape_steps().tolist() == []
    model.run(7)
    assert model.enstape_info["taken"] == 2 and model.enstape("z_plev")[1].shape == (2, 1, 48, 96)
    with pytest.raises(SpeedyHipError, match="not among the configured"):
        model.enstape("u_grid")
    with pytest.raises(SpeedyHipError, match="sample range out of bounds"):
        model.enstape("t_grid", t0=1, nt=2)
    with pytest.raises(SpeedyHipError, match="ensemble tape holds a pressure-level variable"):
        model.plev_configure([700.0])
    assert model.plev_levels == (500.0,)
    buf = torch.empty(16, dtype=torch.float64, device=model.sp.device)
    assert model._lib.spd_model_enstape_read(model._m, b"z_plev", 0, 0, 2, buf.data_ptr(), 128, None) == -3  # SPD_E_SIZE
    assert model._lib.spd_model_enstape_read(model._m, b"z_plev", 3, 0, 2, buf.data_ptr(), 128, None) == -1
    assert b"kind must be" in model._lib.spd_last_error()
    # other names; the levels are free again
    model.enstape_configure(["precnv", "ps_grid"], EVERY, 2)
    model.plev_configure([700.0])
    model.run(8)  # steps 8 ... 15
    assert model.enstape_info["taken"] == 3 and model.enstape_steps().tolist() == [12, 15]
    # a checked call in flight
    stream = model._stream()
    assert model._lib.spd_model_step_checked_begin(model._m, 3, stream) == 0
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.enstape("ps_grid")
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.enstape_configure(["ps_grid"], EVERY, 2)
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.enstape_reset()
    failed = np.zeros(2, dtype=np.int32)
    assert model._lib.spd_model_step_checked_end(model._m, failed.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    assert failed.tolist() == [-1, -1] and model.enstape_steps().tolist() == [15, 18]
    # a member out of range: global-mean temperature of 500 K (diagnostics.f90:57-66), as tests/test_tape_gpu.py
    t = model.get("t", 1)
    t[0, 0, :, :] = 500.0 * np.sqrt(2.0)
    model.set("t", t, member=1)
    failed, _ = model.run_checked(3)
    assert failed.tolist() == [-1, 0]
    with pytest.raises(SpeedyHipError, match="invalid until spd_model_enstape_reset: member 1 failed the range check at step 0"):
        model.enstape("ps_grid")
    assert model.enstape_info["taken"] == 5  # (the count is still told)
    model.enstape_reset()
    assert model.enstape("ps_grid")[0].shape == (0, 48, 96)
    # spd_model_init empties the ring as well
    model.init((1982, 1, 1, 0, 0))
    model.run(6)
    assert model.enstape_info["taken"] == 2 and model.enstape_steps().tolist() == [3, 6]
    model.init((1982, 1, 1, 0, 0))
    assert model.enstape_info["taken"] == 0 and model.enstape_info["capacity"] == 2
    # off: the ring is freed, and nothing samples any more
    model.enstape_configure([], 1, 1)
    with pytest.raises(SpeedyHipError, match="no ensemble tape configured"):
        model.enstape("t_grid")
    model.run(3)
    model.close()
