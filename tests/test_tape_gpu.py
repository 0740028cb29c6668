"""GPU tier: time series of fields recorded on the device inside multi-step calls (spd_model_tape_*, EnsembleModel.tape_*).

The arbiter is the loop a user writes without the tape: a twin model built by the same seeded perturbation as
tests/test_stats_gpu.py (t_grid += N(0, 0.01 K), seed = member id), stepped in calls of `every` steps; after each call
spectral2grid(), the device views of the sigma-level and precipitation variables, and plev().  Every comparison is BITWISE: an fp64
tape equals the twin's fp64 values, an fp32 tape their .float() (DESIGN sections 4a / 4b make the same claims for a sample of the
statistics, 4c for the tape)."""
from datetime import datetime, timedelta

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIGMA = ("u_grid", "v_grid", "t_grid", "q_grid", "phi_grid", "ps_grid", "precnv", "precls")
PLEV = ("u_plev", "v_plev", "t_plev", "q_plev", "z_plev", "mslp")
ALL = SIGMA + PLEV
LEVELS = [1000.0, 850.0, 500.0, 200.0, 10.0]  # hPa: under the ground in places (1000, 850), one above the top full level (10)
EVERY = 9
CALLS = (36, 36, 20)  # samples inside calls and at their ends; steps 91, 92 after the last sample
STATE = ("vor", "div", "t", "tr", "ps")


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


def perturbed(spectral, bc, M, fp32=False, options=(), levels=LEVELS):
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
    views = {n: model.device_view(n) for n in SIGMA}
    if levels:
        model.plev_configure(levels)
    return model, views


def step(model, n, checked=False):
    if checked:
        failed, _ = model.run_checked(n)
        assert (failed == -1).all()
    else:
        model.run(n)


def twin_series(spectral, bc, M, samples, names=ALL, fp32=False, options=(), every=EVERY, tail=0):
    """{name: fp64 tensor [M][samples][levels][48][96] on the device} of the hand-rolled loop, and the spectral state after `tail`
    further steps."""
    import torch
    model, views = perturbed(spectral, bc, M, fp32, options)
    series = {n: [] for n in names}
    for _ in range(samples):
        model.run(every)
        model.spectral2grid()
        for n in names:
            if n in SIGMA:
                series[n].append(views[n].double().clone())
        wanted = [n for n in names if n in PLEV]
        if wanted:
            for n, x in model.plev(wanted).items():
                series[n].append(x.clone())
    assert model.current_step == samples * every
    if tail:
        model.run(tail)
    torch.cuda.synchronize()
    state = {n: [model.get(n, i) for i in range(M)] for n in STATE}
    model.close()
    return {n: torch.stack(v, dim=1) for n, v in series.items()}, state


@pytest.fixture(scope="module")
def twin8(spectral, bc):
    """ten samples of all fourteen names for 8 members in the default plan, and the state after step 92"""
    return twin_series(spectral, bc, 8, 10, tail=2)


def assert_bitwise(got, ref, what):
    import torch
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if not torch.equal(got, ref):
        bad = got != ref
        raise AssertionError("%s: %d of %d values differ, max |diff| %.3e" % (
            what, int(bad.sum()), bad.numel(), float((got.double() - ref.double()).abs().max())))


PLANS = {
    "serial_8": dict(M=8, calls=CALLS),
    "groups_offset_64": dict(M=64, calls=CALLS),
    "rounds_32": dict(M=32, calls=CALLS, options=(("block_members", 4),), checked=True),
    "fp32_physics_8": dict(M=8, calls=CALLS, fp32=True),
    "one_step_calls_8": dict(M=8, calls=(1,) * 92),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_tape_equals_the_hand_rolled_loop(spectral, bc, twin8, plan):
    """All fourteen names at five levels, ten samples every 9 steps over calls of 36, 36 and 20 steps: the fp64 tape is bitwise the
    twin's series and the fp32 tape its .float(), and the recording model's spectral state after step 92 is bitwise the twin's --
    in the serial plan, with two member groups and the offset (64 members), in rounds of block_members (checked calls), with fp32
    physics storage, and in calls of one step."""
    import torch
    p = PLANS[plan]
    M, options, fp32, checked = p["M"], p.get("options", ()), p.get("fp32", False), p.get("checked", False)
    total = sum(p["calls"])
    samples = total // EVERY
    if M == 8 and not fp32 and not options:
        series, twin_state = twin8
    else:
        series, twin_state = twin_series(spectral, bc, M, samples, fp32=fp32, options=options, tail=total - samples * EVERY)
    for dtype, torch_dtype in (("float64", torch.float64), ("float32", torch.float32)):
        model, _ = perturbed(spectral, bc, M, fp32, options)
        model.tape_configure(ALL, EVERY, samples, dtype=dtype)
        cfg = model.config()
        if plan == "groups_offset_64":
            assert cfg["chunks"] == 2
        if plan == "rounds_32":
            assert cfg["rounds"] > 1
        if plan == "fp32_physics_8":
            assert cfg["physics_storage32"]
        for n in p["calls"]:
            step(model, n, checked)
        assert model.current_step == total
        info = model.tape_info
        assert (info["taken"], info["held"], info["capacity"], info["every"], info["dtype"]) == (samples, samples, samples, EVERY, dtype)
        assert model.tape_steps().tolist() == [EVERY * (k + 1) for k in range(samples)]
        for n in ALL:
            got = model.tape(n)
            assert got.dtype == torch_dtype
            assert_bitwise(got, series[n].to(torch_dtype), "%s %s %s" % (plan, dtype, n))
        assert float(series["t_grid"][0].std()) > 0.0 and not torch.equal(series["z_plev"][0], series["z_plev"][1])
        for n, per_member in twin_state.items():
            for i in range(M):
                assert np.array_equal(model.get(n, i), per_member[i]), (plan, dtype, n, i)
        model.close()


def test_the_ring_keeps_the_last_samples(spectral, bc, twin8):
    """Capacity 4, ten samples: the four held ones are the twin's samples 7 to 10 in order; reads in two halves and of a member
    sub-range give the matching slices."""
    import torch
    series, _ = twin8
    names = ("t_grid", "ps_grid", "precls", "z_plev", "mslp")
    model, _ = perturbed(spectral, bc, 8)
    model.tape_configure(names, EVERY, 4)
    for n in CALLS:
        model.run(n)
    info = model.tape_info
    assert (info["taken"], info["held"], info["capacity"], info["dtype"]) == (10, 4, 4, "float32")
    assert model.tape_steps().tolist() == [63, 72, 81, 90]
    for n in names:
        whole = model.tape(n)
        assert_bitwise(whole, series[n][:, 6:10].float(), n)
        halves = torch.cat([model.tape(n, t0=0, nt=2), model.tape(n, t0=2, nt=2)], dim=1)
        assert_bitwise(halves, whole, n + " in two halves")
        assert_bitwise(model.tape(n, first=3, count=2), whole[3:5], n + " members 3, 4")
        assert_bitwise(model.tape(n, first=5, count=3, t0=1, nt=2), whole[5:8, 1:3], n + " members 5 ... 7, samples 1, 2")
    # a ring that is not full yet, and one that has wrapped more than once
    model.tape_reset()
    model.run(20)  # steps 93 ... 112: samples at 99 and 108
    assert model.tape_steps().tolist() == [99, 108] and model.tape("mslp").shape == (8, 2, 48, 96)
    model.close()
    model, _ = perturbed(spectral, bc, 8)
    model.tape_configure(("mslp", "precls"), EVERY, 3, dtype="float64")
    for n in CALLS:
        model.run(n)
    assert model.tape_steps().tolist() == [72, 81, 90]
    assert_bitwise(model.tape("mslp"), series["mslp"][:, 7:10], "mslp, capacity 3")
    assert_bitwise(model.tape("precls"), series["precls"][:, 7:10], "precls, capacity 3")
    model.close()


def test_times(spectral, bc):
    """From 1982-01-01 00:00 with every 9: 06:00, 12:00, 18:00, 00:00 of the next day and so on; the rows of the C ABI carry the
    step counter and the same date."""
    model, _ = perturbed(spectral, bc, 2, levels=None)
    model.tape_configure(["ps_grid"], EVERY, 16)
    model.run(36)
    model.run(20)
    start = datetime(1982, 1, 1)
    assert model.tape_times() == [start + timedelta(hours=6 * k) for k in range(1, 7)]
    assert model.tape_times()[3] == datetime(1982, 1, 2, 0, 0)
    assert model.tape_steps().tolist() == [9, 18, 27, 36, 45, 54]
    rows = np.zeros((4, 6), dtype=np.int32)
    assert model._lib.spd_model_tape_times(model._m, rows.ctypes.data_as(C.POINTER(C.c_int32)), 4) == 4  # (the oldest four)
    assert rows.tolist() == [[9, 1982, 1, 1, 6, 0], [18, 1982, 1, 1, 12, 0], [27, 1982, 1, 1, 18, 0], [36, 1982, 1, 2, 0, 0]]
    # a ring that wrapped: the rows follow their samples
    model.tape_configure(["ps_grid"], EVERY, 2)
    model.run(27)  # steps 57 ... 83: samples at 63, 72, 81
    assert model.tape_steps().tolist() == [72, 81]
    assert model.tape_times() == [start + timedelta(hours=48), start + timedelta(hours=54)]
    model.close()


def test_statistics_and_tape_are_independent(spectral, bc):
    """Statistics every 12 and the tape every 9 on one model: each result is bitwise what it is with the other off, and the final
    state -- every registry variable -- is bitwise that of a run with neither."""
    import torch
    M = 8
    stat_names = ("u_grid", "t_grid", "precnv", "z_plev", "mslp")
    tape_names = ("v_grid", "q_grid", "precnv", "precls", "t_plev", "z_plev")
    runs = {}
    for key, with_stats, with_tape in (("neither", False, False), ("stats", True, False), ("tape", False, True), ("both", True, True)):
        model, _ = perturbed(spectral, bc, M)
        if with_stats:
            model.stats_configure(stat_names, 12, variance=True)
        if with_tape:
            model.tape_configure(tape_names, EVERY, 10, dtype="float64")
        for n in CALLS:
            model.run(n)
        out = {"state": {n: [model.get(n, i) for i in range(M)] for n in model.variables() if n not in ("lon", "lat", "lev")}}
        if with_stats:
            assert model.stats_samples == 7
            out["stats"] = {n: (model.stats_mean(n).clone(), model.stats_var(n).clone()) for n in stat_names}
        if with_tape:
            assert model.tape_info["taken"] == 10
            out["tape"] = {n: model.tape(n).clone() for n in tape_names}
        torch.cuda.synchronize()
        runs[key] = out
        model.close()
    for n in stat_names:
        assert_bitwise(runs["both"]["stats"][n][0], runs["stats"]["stats"][n][0], "mean of " + n)
        assert_bitwise(runs["both"]["stats"][n][1], runs["stats"]["stats"][n][1], "variance of " + n)
    for n in tape_names:
        assert_bitwise(runs["both"]["tape"][n], runs["tape"]["tape"][n], "tape of " + n)
    for key in ("stats", "tape", "both"):
        for n, per_member in runs["neither"]["state"].items():
            for a, b in zip(per_member, runs[key]["state"][n]):
                assert np.array_equal(a, b), (key, n)


def test_lifecycle(spectral, bc):
    """Reads before configuring and of unconfigured names fail; reset empties; a reconfiguration changes names and dtype; init
    empties; plev_configure is refused while a pressure-level name is held; reads are refused while a checked call is in flight;
    a checked call that reports a failed range check makes reads fail, naming member and step, until the next reset; off frees."""
    import torch
    from pyspeedy_amd._lib import SpeedyHipError
    model, views = perturbed(spectral, bc, 2, levels=None)
    with pytest.raises(SpeedyHipError, match="no tape configured"):
        model.tape_info
    with pytest.raises(SpeedyHipError, match="no tape configured"):
        model.tape_reset()
    with pytest.raises(SpeedyHipError, match="unknown variable"):
        model.tape_configure(["t_grid", "olr"], EVERY, 4)
    with pytest.raises(SpeedyHipError, match="every"):
        model.tape_configure(["t_grid"], 0, 4)
    with pytest.raises(SpeedyHipError, match="capacity"):
        model.tape_configure(["t_grid"], EVERY, 0)
    with pytest.raises(ValueError, match="dtype"):
        model.tape_configure(["t_grid"], EVERY, 4, dtype="float16")
    with pytest.raises(SpeedyHipError, match="needs target levels"):
        model.tape_configure(["t_grid", "z_plev"], EVERY, 4)
    model.plev_configure([500.0])
    model.tape_configure(["t_grid", "z_plev"], 3, 4)
    assert model.tape_info == dict(taken=0, held=0, capacity=4, every=3, dtype="float32")
    assert model.tape("t_grid").shape == (2, 0, 8, 48, 96) and model.tape_steps().tolist() == [] and model.tape_times() == []
    model.run(7)
    assert model.tape_info["taken"] == 2 and model.tape("t_grid").dtype == torch.float32
    with pytest.raises(SpeedyHipError, match="not among the configured"):
        model.tape("u_grid")
    with pytest.raises(SpeedyHipError, match="sample range out of bounds"):
        model.tape("t_grid", t0=1, nt=2)
    with pytest.raises(SpeedyHipError, match="member range out of bounds"):
        model.tape("t_grid", first=1, count=2)
    with pytest.raises(SpeedyHipError, match="tape holds a pressure-level variable"):
        model.plev_configure([700.0])
    assert model.plev_levels == (500.0,)
    buf = torch.empty(8, dtype=torch.float32, device=model.sp.device)
    assert model._lib.spd_model_tape_read(model._m, b"z_plev", 0, 2, 0, 2, buf.data_ptr(), 32, None) == -3  # SPD_E_SIZE
    model.tape_reset()
    assert model.tape_info["taken"] == 0 and model.tape_info["held"] == 0
    model.run(2)  # step 9: one sample, which is what the export gives now
    model.spectral2grid()
    assert model.tape_steps().tolist() == [9]
    assert torch.equal(model.tape("t_grid")[:, 0], views["t_grid"].float())
    # other names, the other dtype
    model.tape_configure(["precnv", "ps_grid"], 3, 2, dtype="float64")
    assert model.tape_info == dict(taken=0, held=0, capacity=2, every=3, dtype="float64")
    model.plev_configure([700.0])  # (no pressure-level name is held any more)
    model.run(9)
    assert model.tape_info["taken"] == 3 and model.tape_steps().tolist() == [15, 18]
    assert model.tape("ps_grid").dtype == torch.float64 and model.tape("ps_grid").shape == (2, 2, 48, 96)
    with pytest.raises(SpeedyHipError, match="not among the configured"):
        model.tape("t_grid")
    # a checked call in flight
    stream = model._stream()
    assert model._lib.spd_model_step_checked_begin(model._m, 3, stream) == 0
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.tape("ps_grid")
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.tape_configure(["ps_grid"], 3, 2)
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.tape_reset()
    failed = np.zeros(2, dtype=np.int32)
    assert model._lib.spd_model_step_checked_end(model._m, failed.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    assert failed.tolist() == [-1, -1] and model.tape_steps().tolist() == [18, 21]
    # a member out of range: global-mean temperature of 500 K (diagnostics.f90:57-66), as tests/test_stats_gpu.py
    t = model.get("t", 1)
    t[0, 0, :, :] = 500.0 * np.sqrt(2.0)
    model.set("t", t, member=1)
    failed, _ = model.run_checked(3)
    assert failed.tolist() == [-1, 0]
    with pytest.raises(SpeedyHipError, match="invalid until spd_model_tape_reset: member 1 failed the range check at step 0"):
        model.tape("ps_grid")
    assert model.tape_info["taken"] == 5  # (the count is still told)
    model.tape_reset()
    assert model.tape("ps_grid").shape == (2, 0, 48, 96)
    # spd_model_init empties the tape as well (set_bc ends in it)
    model.init((1982, 1, 1, 0, 0))
    model.run(6)
    assert model.tape_info["taken"] == 2 and model.tape_steps().tolist() == [3, 6]
    model.init((1982, 1, 1, 0, 0))
    assert model.tape_info["taken"] == 0 and model.tape_info["capacity"] == 2
    # off
    model.tape_configure([], 1, 1)
    with pytest.raises(SpeedyHipError, match="no tape configured"):
        model.tape("ps_grid")
    model.run(3)
    model.close()


def test_shapes_dtypes_and_device(spectral, bc):
    """Everything tape() returns: [count][nt][levels][48][96] ([count][nt][48][96] for one-level names) in the tape's dtype on the
    model's device."""
    import torch
    for dtype, torch_dtype in (("float32", torch.float32), ("float64", torch.float64)):
        model, _ = perturbed(spectral, bc, 3, levels=[850.0, 500.0])
        model.tape_configure(ALL, EVERY, 3, dtype=dtype)
        model.run(20)
        device = model.device_view("t_grid").device
        for n in ALL:
            inner = (8, 48, 96) if n in SIGMA[:5] else (2, 48, 96) if n in PLEV[:5] else (48, 96)
            x = model.tape(n)
            assert x.shape == (3, 2) + inner and x.dtype == torch_dtype and x.device == device and x.is_contiguous(), n
            y = model.tape(n, first=1, count=2, t0=1, nt=1)
            assert y.shape == (2, 1) + inner and y.dtype == torch_dtype and y.device == device, n
            assert torch.equal(y, x[1:3, 1:2]), n
            assert bool(torch.isfinite(x).all()), n
        assert isinstance(model.tape_steps(), np.ndarray) and model.tape_steps().dtype.kind == "i"
        assert all(isinstance(t, datetime) for t in model.tape_times())
        model.close()
