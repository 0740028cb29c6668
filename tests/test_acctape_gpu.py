"""GPU tier: window sums, means and extremes of the physics fluxes accumulated on the device behind every step
(spd_model_acctape_*, EnsembleModel.acctape_*).

The arbiter is the loop a user writes without the recorder: a twin model built by the same seeded perturbation as
tests/test_tape_gpu.py (t_grid += N(0, 0.01 K), seed = member id), stepped in CALLS OF ONE STEP -- the last step of a call always
stores the diagnostics-only outputs -- and after each call the device views of the names, as .double().  The windows are reduced by
an explicit loop in step order with exactly the recorder's rules: sum = the first value, then sum + x; min / max = the first value,
then x < acc ? x : acc and x > acc ? x : acc (one elementwise IEEE operation per step and element, on the tensors where they lie; no
np.sum or torch.sum, which add pairwise); mean = that sum / n, divided by numpy on the CPU.  Every comparison is BITWISE: an fp64 ring
equals the arbiter, an fp32 ring its .float().

A member's trajectory does not depend on how many members its model has or on the launch plan, so one twin of 20 members serves
every fp64 case (the cases of 3 members use its first 3) and one twin of 3 members the fp32-storage case."""
from datetime import datetime, timedelta

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ONE = ("precnv", "precls", "cbmf", "olr", "tsr", "ssr", "ssrd", "slr", "slrd")
THREE = ("ustr", "vstr", "shf", "evap", "slru")  # planes: 0 land, 1 sea, 2 weighted by the land fraction
NAMES = ONE + THREE
OPS = ("sum", "mean", "min", "max")
ALL = tuple((n, op) for n in NAMES for op in OPS)
EVERY = 4                   # not a multiple of the shortwave's 3
CALLS = (5, 1, 7, 12, 3)    # 28 steps, 7 windows, most of them across call ends
TOTAL = sum(CALLS)
STATE = ("vor", "div", "t", "tr", "ps")
START = datetime(1982, 1, 1)
# The plane of a three-plane name the emptiness check looks at: 2, the weighted one.  Planes 0 and 1 are what the land and the sea
# surface would give at every point; the land-sea mask enters plane 2 only (x_sea + fmask * (x_land - x_sea)), which is the flux
# the atmosphere sees and the one that is non-trivial at every point whatever the mask says there.
MASKED_PLANE = 2


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
    views = {n: model.device_view(n) for n in NAMES}
    return model, views


def step(model, n, checked=False):
    if checked:
        failed, _ = model.run_checked(n)
        assert (failed == -1).all()
    else:
        model.run(n)


def twin_steps(spectral, bc, M, fp32=False, total=TOTAL):
    """{name: fp64 tensor [total][M][(3,)48][96] on the device}: what the column physics stored in each step of a loop of one-step
    calls; and the spectral state and the stored precnv, olr, shf after the last one."""
    import torch
    model, views = perturbed(spectral, bc, M, fp32)
    if fp32:
        assert model.config()["physics_storage32"] and views["olr"].dtype == torch.float32 and views["tsr"].dtype == torch.float64
    steps = {n: [] for n in NAMES}
    for _ in range(total):
        model.run(1)
        for n in NAMES:
            steps[n].append(views[n].double().clone())
    assert model.current_step == total
    torch.cuda.synchronize()
    final = {n: [model.get(n, i) for i in range(M)] for n in STATE}
    final.update({n: views[n].clone() for n in ("precnv", "olr", "shf")})
    model.close()
    return {n: torch.stack(v) for n, v in steps.items()}, final


def reduce_windows(steps, bounds, members=None, entries=ALL):
    """{(name, op): fp64 tensor [M][windows][(3,)48][96]} for the windows [a, b) of step indices, by the explicit loop."""
    import torch
    out = {}
    sl = slice(None) if members is None else slice(0, members)
    for name in sorted({n for n, _ in entries}):
        x = steps[name][:, sl]
        cols = {op: [] for op in OPS}
        for a, b in bounds:
            s = x[a].clone()
            lo = x[a].clone()
            hi = x[a].clone()
            for k in range(a + 1, b):  # in step order
                s = s + x[k]
                lo = torch.where(x[k] < lo, x[k], lo)
                hi = torch.where(x[k] > hi, x[k], hi)
            cols["sum"].append(s)
            cols["mean"].append(torch.from_numpy(s.cpu().numpy() / np.float64(b - a)).to(s.device))  # one IEEE division
            cols["min"].append(lo)
            cols["max"].append(hi)
        for op in OPS:
            if (name, op) in entries:
                out[(name, op)] = torch.stack(cols[op], dim=1)
    return out


def windows_from(first, total=TOTAL, every=EVERY):
    """[a, b) step indices of the windows a recorder closes that starts at absolute step `first`"""
    edges = [first] + [e for e in range(every, total + 1, every) if e > first]
    return list(zip(edges[:-1], edges[1:]))


@pytest.fixture(scope="module")
def twin20(spectral, bc):
    steps, final = twin_steps(spectral, bc, 20)
    return steps, final, reduce_windows(steps, windows_from(0))


@pytest.fixture(scope="module")
def twin3(twin20):
    """the first 3 members of the twin, with the standard windows"""
    steps, final, ref = twin20
    return steps, final, {k: v[:3] for k, v in ref.items()}


def assert_bitwise(got, ref, what):
    import torch
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if not torch.equal(got, ref):
        bad = got != ref
        raise AssertionError("%s: %d of %d values differ, max |diff| %.3e" % (
            what, int(bad.sum()), bad.numel(), float((got.double() - ref.double()).abs().max())))


def assert_state(model, final, M, what):
    import torch
    for n in STATE:
        for i in range(M):
            assert np.array_equal(model.get(n, i), final[n][i]), (what, n, i)
    for n in ("precnv", "olr", "shf"):
        assert torch.equal(model.device_view(n), final[n][:M]), (what, n)


def test_the_arbiter_is_not_empty(twin20):
    """On the arbiter's own data, per name (plane MASKED_PLANE of a three-plane name): inside at least one window, at some point,
    max > min and sum != n * last value.  A recorder that kept only the last step would otherwise pass every comparison."""
    steps, _, ref = twin20
    bounds = windows_from(0)
    for name in NAMES:
        pick = (lambda x: x[..., MASKED_PLANE, :, :]) if name in THREE else (lambda x: x)
        spread = pick(ref[(name, "max")]) > pick(ref[(name, "min")])  # [M][windows][48][96]
        last = pick(steps[name])[[b - 1 for _, b in bounds]].transpose(0, 1)  # [M][windows][48][96]
        differs = pick(ref[(name, "sum")]) != float(EVERY) * last
        both = spread & differs
        print("%-7s points that vary inside a window: %d of %d" % (name, int(both.sum()), both.numel()))
        assert bool(both.any()), name


PLANS = {
    "serial_3": dict(M=3, calls=CALLS),
    "two_groups_20": dict(M=20, calls=CALLS),
    "rounds_20": dict(M=20, calls=CALLS, options=(("block_members", 4),), checked=True),
    "fp32_storage_3": dict(M=3, calls=CALLS, fp32=True),
    "one_step_calls_3": dict(M=3, calls=(1,) * TOTAL),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_windows_equal_the_hand_rolled_loop(spectral, bc, twin20, plan):
    """All fourteen names under all four ops, 7 windows of 4 steps over calls of 5, 1, 7, 12 and 3 steps: the fp64 ring is bitwise
    the arbiter and the fp32 ring its .float(), steps, dates and counts are right, and the recording model's spectral state and
    stored precnv, olr, shf after step 28 are bitwise the twin's -- serial, with two member groups, in rounds of block_members
    (checked calls), with fp32 physics storage, and in calls of one step."""
    import torch
    p = PLANS[plan]
    M, options, fp32, checked = p["M"], p.get("options", ()), p.get("fp32", False), p.get("checked", False)
    if fp32:
        steps, final = twin_steps(spectral, bc, M, fp32=True)
        ref = reduce_windows(steps, windows_from(0))
    else:
        final, ref = twin20[1], {k: v[:M] for k, v in twin20[2].items()}
    for dtype, torch_dtype in (("float64", torch.float64), ("float32", torch.float32)):
        model, _ = perturbed(spectral, bc, M, fp32, options)
        model.acctape_configure(ALL, EVERY, 7, dtype=dtype)
        cfg = model.config()
        if plan == "serial_3":
            assert cfg["chunks"] == 1 and cfg["rounds"] == 1
        if plan == "two_groups_20":
            assert cfg["chunks"] == 2 and cfg["rounds"] == 1
        if plan == "rounds_20":
            assert cfg["rounds"] > 1
        if plan == "fp32_storage_3":
            assert cfg["physics_storage32"]
        for n in p["calls"]:
            step(model, n, checked)
        assert model.current_step == TOTAL
        info = model.acctape_info
        assert (info["taken"], info["held"], info["capacity"], info["every"], info["dtype"]) == (7, 7, 7, EVERY, dtype)
        assert model.acctape_steps().tolist() == [EVERY * (k + 1) for k in range(7)]
        assert model.acctape_counts().tolist() == [EVERY] * 7
        assert model.acctape_times() == [START + timedelta(minutes=40 * EVERY * (k + 1)) for k in range(7)]
        for name, op in ALL:
            got = model.acctape(name, op)
            assert got.dtype == torch_dtype and got.shape == (M, 7) + ((3, 48, 96) if name in THREE else (48, 96))
            assert_bitwise(got, ref[(name, op)].to(torch_dtype), "%s %s %s %s" % (plan, dtype, name, op))
        assert_state(model, final, M, (plan, dtype))
        model.close()


def test_a_recorder_configured_after_two_steps_starts_a_short_window(spectral, bc, twin3):
    """The first window after _configure starts at the model's current step: n = 2, and acctape_counts() says so."""
    steps, _, _ = twin3
    entries = (("precnv", "sum"), ("olr", "mean"), ("cbmf", "max"), ("evap", "min"))
    model, _ = perturbed(spectral, bc, 3)
    model.run(2)
    model.acctape_configure(entries, EVERY, 8, dtype="float64")
    for n in (3, 1, 7, 12, 3):
        model.run(n)
    assert model.current_step == TOTAL
    bounds = windows_from(2)
    assert bounds[0] == (2, 4) and len(bounds) == 7
    assert model.acctape_counts().tolist() == [2, 4, 4, 4, 4, 4, 4]
    assert model.acctape_steps().tolist() == [4, 8, 12, 16, 20, 24, 28]
    ref = reduce_windows(steps, bounds, members=3, entries=entries)
    for name, op in entries:
        assert_bitwise(model.acctape(name, op), ref[(name, op)], "%s %s" % (name, op))
    model.close()


def test_the_ring_keeps_the_last_windows(spectral, bc, twin3):
    """Capacity 5 with 7 windows taken: 5 are held, oldest first, and steps, dates and counts are right; reads of sub-ranges give
    the matching slices; SPD_E_SIZE for a destination that is too small."""
    import torch
    _, _, ref = twin3
    entries = (("precls", "sum"), ("tsr", "mean"), ("shf", "max"))
    model, _ = perturbed(spectral, bc, 3)
    model.acctape_configure(entries, EVERY, 5)
    for n in CALLS:
        model.run(n)
    info = model.acctape_info
    assert (info["taken"], info["held"], info["capacity"], info["dtype"]) == (7, 5, 5, "float32")
    assert model.acctape_steps().tolist() == [12, 16, 20, 24, 28]
    assert model.acctape_counts().tolist() == [4] * 5
    assert model.acctape_times() == [START + timedelta(minutes=40 * s) for s in (12, 16, 20, 24, 28)]
    rows = np.zeros((2, 7), dtype=np.int32)
    assert model._lib.spd_model_acctape_times(model._m, rows.ctypes.data_as(C.POINTER(C.c_int32)), 2) == 2  # (the oldest two)
    assert rows.tolist() == [[12, 1982, 1, 1, 8, 0, 4], [16, 1982, 1, 1, 10, 40, 4]]
    for name, op in entries:
        whole = model.acctape(name, op)
        assert_bitwise(whole, ref[(name, op)][:, 2:7].float(), "%s %s" % (name, op))
        halves = torch.cat([model.acctape(name, op, t0=0, nt=2), model.acctape(name, op, t0=2, nt=3)], dim=1)
        assert_bitwise(halves, whole, name + " in two parts")
        assert_bitwise(model.acctape(name, op, first=1, count=2, t0=3, nt=1), whole[1:3, 3:4], name + " members 1, 2, window 3")
    buf = torch.empty(8, dtype=torch.float32, device=model.sp.device)
    assert model._lib.spd_model_acctape_read(model._m, b"tsr", 1, 0, 3, 0, 5, buf.data_ptr(), 32, None) == -3  # SPD_E_SIZE
    model.close()


def test_reset_reconfigure_and_off(spectral, bc, twin3):
    """_reset in mid-window starts a short window; reconfiguring with other entries; a three-plane name returns the registry's
    three planes in order; _configure with 0 entries, after which _read fails with its reason."""
    import torch
    from pyspeedy_amd._lib import SpeedyHipError
    steps, _, _ = twin3
    first = (("precnv", "max"), ("ustr", "mean"))
    model, _ = perturbed(spectral, bc, 3)
    with pytest.raises(SpeedyHipError, match="no accumulation tape configured"):
        model.acctape_info
    model.acctape_configure(first, EVERY, 4, dtype="float64")
    assert model.acctape_info == dict(taken=0, held=0, capacity=4, every=EVERY, dtype="float64")
    assert model.acctape("ustr", "mean").shape == (3, 0, 3, 48, 96) and model.acctape_counts().tolist() == []
    model.run(6)
    assert model.acctape_steps().tolist() == [4]
    model.acctape_reset()  # at step 6: the open window (steps 5, 6) is dropped, the next one holds steps 7 and 8
    assert model.acctape_info["taken"] == 0
    model.run(6)
    assert model.acctape_steps().tolist() == [8, 12] and model.acctape_counts().tolist() == [2, 4]
    ref = reduce_windows(steps, [(6, 8), (8, 12)], members=3, entries=first)
    for name, op in first:
        assert_bitwise(model.acctape(name, op), ref[(name, op)], "after reset: %s %s" % (name, op))
    with pytest.raises(SpeedyHipError, match="not among the configured entries"):
        model.acctape("precnv", "sum")
    with pytest.raises(SpeedyHipError, match="window range out of bounds"):
        model.acctape("precnv", "max", t0=1, nt=2)
    with pytest.raises(SpeedyHipError, match="member range out of bounds"):
        model.acctape("precnv", "max", first=2, count=2)
    with pytest.raises(ValueError, match="op must be"):
        model.acctape("precnv", "median")
    # other entries, the other dtype, another window length: configured at step 12
    second = (("shf", "sum"), ("shf", "min"), ("slrd", "mean"))
    model.acctape_configure(second, 8, 3)
    assert model.acctape_info == dict(taken=0, held=0, capacity=3, every=8, dtype="float32")
    model.run(12)  # steps 13 ... 24: windows (12, 16] and (16, 24]
    assert model.acctape_steps().tolist() == [16, 24] and model.acctape_counts().tolist() == [4, 8]
    ref = reduce_windows(steps, [(12, 16), (16, 24)], members=3, entries=second)
    for name, op in second:
        assert_bitwise(model.acctape(name, op), ref[(name, op)].float(), "reconfigured: %s %s" % (name, op))
    with pytest.raises(SpeedyHipError, match="not among the configured entries"):
        model.acctape("ustr", "mean")
    # the three planes of shf in the registry's order: land, sea, weighted
    got = model.acctape("shf", "sum")
    for k in range(3):
        x = steps["shf"][12:16, :3, k]
        s = x[0].clone()
        for j in range(1, 4):
            s = s + x[j]
        assert_bitwise(got[:, 0, k], s.float(), "shf plane %d" % k)
    assert not torch.equal(got[:, 0, 0], got[:, 0, 1]) and not torch.equal(got[:, 0, 1], got[:, 0, 2])
    # off
    model.acctape_configure([], 1, 1)
    with pytest.raises(SpeedyHipError, match="no accumulation tape configured"):
        model.acctape("shf", "sum")
    with pytest.raises(SpeedyHipError, match="no accumulation tape configured"):
        model.acctape_reset()
    model.run(3)
    model.close()


def test_checked_calls_init_and_validity(spectral, bc):
    """Configuration, reset and reads are refused while a checked call is in flight; a checked call that reports a failed range
    check makes reads fail, naming member and step, until the next reset; spd_model_init empties the ring and starts a window."""
    from pyspeedy_amd._lib import SpeedyHipError
    model, _ = perturbed(spectral, bc, 2)
    model.acctape_configure([("olr", "mean")], 3, 2, dtype="float64")
    stream = model._stream()
    assert model._lib.spd_model_step_checked_begin(model._m, 4, stream) == 0
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.acctape("olr", "mean")
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.acctape_configure([("olr", "mean")], 3, 2)
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.acctape_reset()
    failed = np.zeros(2, dtype=np.int32)
    assert model._lib.spd_model_step_checked_end(model._m, failed.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    assert failed.tolist() == [-1, -1] and model.acctape_steps().tolist() == [3]
    # a member out of range: global-mean temperature of 500 K (diagnostics.f90:57-66), as tests/test_tape_gpu.py
    t = model.get("t", 1)
    t[0, 0, :, :] = 500.0 * np.sqrt(2.0)
    model.set("t", t, member=1)
    failed, _ = model.run_checked(3)
    assert failed.tolist() == [-1, 0]
    with pytest.raises(SpeedyHipError, match="invalid until spd_model_acctape_reset: member 1 failed the range check at step 0"):
        model.acctape("olr", "mean")
    assert model.acctape_info["taken"] == 2  # (the count is still told)
    model.acctape_reset()
    assert model.acctape("olr", "mean").shape == (2, 0, 48, 96)
    model.init((1982, 1, 1, 0, 0))
    model.run(7)
    assert model.acctape_steps().tolist() == [3, 6] and model.acctape_counts().tolist() == [3, 3]
    model.init((1982, 1, 1, 0, 0))
    assert model.acctape_info["taken"] == 0 and model.acctape_info["capacity"] == 2
    model.close()


def test_the_recorders_are_independent(spectral, bc, twin3):
    """The accumulation tape gives bitwise the same with the tape and the ensemble tape (both holding precnv) on beside it as alone,
    they give the same as without it, and the final state -- every registry variable -- is bitwise that of a run with none."""
    import torch
    M = 3
    entries = (("precnv", "sum"), ("precnv", "max"), ("olr", "mean"), ("vstr", "min"))
    runs = {}
    for key, with_acc, with_others in (("none", False, False), ("acc", True, False), ("others", False, True), ("all", True, True)):
        model, _ = perturbed(spectral, bc, M)
        if with_others:
            model.tape_configure(["precnv", "t_grid"], 3, 9, dtype="float64")
            model.enstape_configure(["precnv", "ps_grid"], 6, 4)
        if with_acc:
            model.acctape_configure(entries, EVERY, 7, dtype="float64")
        for n in CALLS:
            model.run(n)
        out = {"state": {n: [model.get(n, i) for i in range(M)] for n in model.variables() if n not in ("lon", "lat", "lev")}}
        if with_others:
            assert model.tape_info["taken"] == 9 and model.enstape_info["taken"] == 4
            out["tape"] = {n: model.tape(n).clone() for n in ("precnv", "t_grid")}
            out["enstape"] = {n: tuple(x.clone() for x in model.enstape(n)) for n in ("precnv", "ps_grid")}
        if with_acc:
            assert model.acctape_info["taken"] == 7
            out["acc"] = {e: model.acctape(*e).clone() for e in entries}
        torch.cuda.synchronize()
        runs[key] = out
        model.close()
    for e in entries:
        assert_bitwise(runs["all"]["acc"][e], runs["acc"]["acc"][e], "beside the others: %s %s" % e)
        assert_bitwise(runs["acc"]["acc"][e], twin3[2][e], "alone: %s %s" % e)
    for n in ("precnv", "t_grid"):
        assert_bitwise(runs["all"]["tape"][n], runs["others"]["tape"][n], "tape of " + n)
    for n in ("precnv", "ps_grid"):
        for a, b, what in zip(runs["all"]["enstape"][n], runs["others"]["enstape"][n], ("mean", "std")):
            assert_bitwise(a, b, "ensemble tape %s of %s" % (what, n))
    for key in ("acc", "others", "all"):
        for n, per_member in runs["none"]["state"].items():
            for a, b in zip(per_member, runs[key]["state"][n]):
                assert np.array_equal(a, b), (key, n)
