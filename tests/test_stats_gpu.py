"""GPU tier: time-mean statistics accumulated on the device inside multi-step calls (spd_model_stats_*, EnsembleModel.stats_*).

The reference for every statistic is the loop a user writes by hand without them (tests/test_long_gpu.py): a twin model stepped
in calls of `every` steps, spectral2grid() and an fp64 read of every variable after each call, averaged on the host.  Members are
the seeded perturbations of test_long_gpu.py (t_grid += N(0, 0.01 K), seed = member id)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VARS = ("u_grid", "v_grid", "t_grid", "q_grid", "phi_grid", "ps_grid", "precnv", "precls")
EVERY = 9


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


def perturbed(spectral, bc, M, fp32=False, options=()):
    import torch
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, M)
    model.set_bc(bc, start_date=(1982, 1, 1, 0, 0))
    for name, value in options:
        model.set_option(name, value)
    if fp32:
        model.set_physics_precision(True)
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng(i).normal(0.0, 0.01, (96, 48, 8)).transpose(2, 1, 0) for i in range(M)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()
    # (every view the twin reads through is taken now, on both models alike: taking a view drops derived state)
    views = {n: model.device_view(n) for n in VARS}
    return model, views


def step(model, n, checked):
    if checked:
        failed, _ = model.run_checked(n)
        assert (failed == -1).all()
    else:
        model.run(n)


def twin_statistics(spectral, bc, M, samples, fp32=False, options=()):
    """Means and variances of `samples` hand-rolled samples: calls of EVERY steps, spectral2grid, fp64 reads to the host,
    shifted sums (the first sample as shift) in numpy."""
    import torch
    model, views = perturbed(spectral, bc, M, fp32, options)
    shift, s1, s2 = {}, {}, {}
    for k in range(samples):
        model.run(EVERY)
        model.spectral2grid()
        torch.cuda.synchronize()
        for n in VARS:
            x = views[n].double().cpu().numpy()
            if k == 0:
                shift[n], s1[n], s2[n] = x, np.zeros_like(x), np.zeros_like(x)
            d = x - shift[n]
            s1[n] += d
            s2[n] += d * d
    assert model.current_step == samples * EVERY
    mean = {n: shift[n] + s1[n] / samples for n in VARS}
    var = {n: (s2[n] - s1[n] * s1[n] / samples) / (samples - 1) for n in VARS}
    state = {n: [model.get(n, i) for i in range(M)] for n in ("vor", "div", "t", "tr", "ps")}
    model.close()
    return mean, var, state


def scaled(got, ref):
    return float(np.abs(got - ref).max() / max(float(ref.max() - ref.min()), 1e-300))


def check_against_twin(model, mean, var, samples):
    assert model.stats_samples == samples
    worst = {}
    for n in VARS:
        em = scaled(model.stats_mean(n).cpu().numpy(), mean[n])
        ev = scaled(model.stats_var(n).cpu().numpy(), var[n])
        worst[n] = (em, ev)
        assert em <= 1e-12 and ev <= 1e-12, (n, em, ev)
    return worst


# calls of 36, 36 and 20 steps: samples inside calls and at their ends; steps 90 ... 92 after the last sample
PLANS = {
    "serial_8": dict(M=8, calls=(36, 36, 20)),
    "groups_offset_64": dict(M=64, calls=(36, 36, 20)),
    "rounds_32": dict(M=32, calls=(36, 36, 20), options=(("block_members", 4),), checked=True),
    "fp32_physics_8": dict(M=8, calls=(36, 36, 20), fp32=True),
    "one_step_calls_8": dict(M=8, calls=(1,) * 92),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_statistics_equal_the_hand_rolled_loop(spectral, bc, plan):
    """Means and variances of all 8 variables agree with the twin's to 1e-12 of each field's range, and the sampling model's
    spectral state is bitwise the twin's -- in the serial plan, with two member groups and the 3/4-step offset (64 members),
    in rounds of block_members (through checked calls), with fp32 physics storage, and in calls of one step."""
    p = PLANS[plan]
    M, options, fp32, checked = p["M"], p.get("options", ()), p.get("fp32", False), p.get("checked", False)
    samples = sum(p["calls"]) // EVERY
    mean, var, twin_state = twin_statistics(spectral, bc, M, samples, fp32, options)
    model, _ = perturbed(spectral, bc, M, fp32, options)
    model.stats_configure(VARS, EVERY, variance=True)
    cfg = model.config()
    if plan == "groups_offset_64":
        assert cfg["chunks"] == 2
    if plan == "rounds_32":
        assert cfg["rounds"] > 1
    if plan == "fp32_physics_8":
        assert cfg["physics_storage32"]
    for n in p["calls"]:
        step(model, n, checked)
    assert model.current_step == sum(p["calls"])
    worst = check_against_twin(model, mean, var, samples)
    print(plan, {n: "%.1e / %.1e" % w for n, w in worst.items()})
    model.close()
    # the twin stopped at the last sample; the spectral state there is the sampling model's after the same steps
    model, _ = perturbed(spectral, bc, M, fp32, options)
    model.stats_configure(VARS, EVERY, variance=True)
    left = samples * EVERY
    for n in p["calls"]:
        n = min(n, left)
        if n:
            step(model, n, checked)
        left -= n
    for n, per_member in twin_state.items():
        for i in range(M):
            assert np.array_equal(model.get(n, i), per_member[i]), (n, i)
    model.close()


def test_sampling_changes_nothing_of_the_run(spectral, bc):
    """After the same calls the spectral state and EVERY registry variable -- u_grid ... ps_grid included, which sampling must not
    write -- are bitwise those of a model without statistics."""
    M, calls = 8, (36, 36, 20)
    states = []
    for with_stats in (False, True):
        model, _ = perturbed(spectral, bc, M)
        if with_stats:
            model.stats_configure(VARS, EVERY, variance=True)
        for n in calls:
            model.run(n)
        if with_stats:
            assert model.stats_samples == 10
        states.append({n: [model.get(n, i) for i in range(M)] for n in model.variables() if n not in ("lon", "lat", "lev")})
        model.close()
    for n, per_member in states[0].items():
        for a, b in zip(per_member, states[1][n]):
            assert np.array_equal(a, b), n


def test_ensemble_reduction(spectral, bc):
    """stats_ensemble: the members' time means averaged (and their ddof-1 spread) per point, on the device, against torch."""
    import torch
    model, _ = perturbed(spectral, bc, 8)
    model.stats_configure(VARS, EVERY, variance=False)
    model.run(36)
    for n in VARS:
        per_member = model.stats_mean(n)
        mean, std = model.stats_ensemble(n)
        ref_mean, ref_std = torch.mean(per_member, dim=0), torch.std(per_member, dim=0, unbiased=True)
        assert mean.shape == ref_mean.shape == per_member.shape[1:]
        # (both against the size of the values reduced: members' means of 250 K are known to 250 K x 2.2e-16 only, and two
        # summation orders make a spread of 1e-3 K differ by that much)
        scale = float(per_member.abs().max())
        assert float((mean - ref_mean).abs().max()) <= 1e-13 * scale, n
        assert float((std - ref_std).abs().max()) <= 1e-13 * scale, n
        assert float(ref_std.max()) > 0.0, n  # (the members differ)
    model.close()


def test_lifecycle(spectral, bc):
    """Reads before configuring and of unconfigured names fail; reset restarts the count (the next sample is the whole mean);
    a reconfiguration changes the variables; a checked call that reports a failed range check (-2, an out-of-range state set from
    the host) makes reads fail until the next reset."""
    import torch
    from pyspeedy_amd._lib import SpeedyHipError
    model, views = perturbed(spectral, bc, 2)
    with pytest.raises(SpeedyHipError, match="no statistics configured"):
        model.stats_mean("t_grid")
    with pytest.raises(SpeedyHipError, match="no statistics configured"):
        model.stats_samples
    with pytest.raises(SpeedyHipError, match="unknown variable"):
        model.stats_configure(["t_grid", "olr"], EVERY)
    with pytest.raises(SpeedyHipError, match="every"):
        model.stats_configure(["t_grid"], 0)
    model.stats_configure(["t_grid"], EVERY, variance=False)
    with pytest.raises(SpeedyHipError, match="no sample"):
        model.stats_mean("t_grid")
    model.run(20)
    assert model.stats_samples == 2
    with pytest.raises(SpeedyHipError, match="not among the configured"):
        model.stats_mean("u_grid")
    with pytest.raises(SpeedyHipError, match="without variance"):
        model.stats_var("t_grid")
    model.stats_reset()
    assert model.stats_samples == 0
    model.run(7)  # step 27: one sample, which is then the whole period
    assert model.stats_samples == 1
    model.spectral2grid()
    assert torch.equal(model.stats_mean("t_grid"), views["t_grid"])
    model.stats_configure(["precnv", "ps_grid"], 3, variance=True)
    assert model.stats_samples == 0
    model.run(6)
    assert model.stats_samples == 2
    with pytest.raises(SpeedyHipError, match="not among the configured"):
        model.stats_mean("t_grid")
    assert model.stats_var("ps_grid").shape == (2, 48, 96)
    # a member out of range: global-mean temperature of 500 K (diagnostics.f90:57-66)
    t = model.get("t", 1)
    t[0, 0, :, :] = 500.0 * np.sqrt(2.0)
    model.set("t", t, member=1)
    failed, _ = model.run_checked(3)
    assert failed.tolist() == [-1, 0]
    with pytest.raises(SpeedyHipError, match="invalid"):
        model.stats_mean("ps_grid")
    with pytest.raises(SpeedyHipError, match="invalid"):
        model.stats_ensemble("ps_grid")
    model.stats_reset()
    with pytest.raises(SpeedyHipError, match="no sample"):
        model.stats_mean("ps_grid")
    # spd_model_init starts a new period as well
    model.init((1982, 1, 1, 0, 0))
    model.run(3)
    assert model.stats_samples == 1 and model.stats_mean("precnv").shape == (2, 48, 96)
    model.close()
