"""GPU tier: window sums, means, extremes and threshold counts of the state's fields accumulated on the device
(spd_model_wintape_*, EnsembleModel.wintape_*).

The arbiter is existing code: a twin model built by the same seeded perturbation as tests/test_tape_gpu.py (t_grid += N(0, 0.01 K),
seed = member id) that holds an fp64 TAPE of the needed names with every = the recorder's sample_every.  Its samples are reduced
window by window in sample order with exactly the recorder's rules: sum = the first sample, then sum + x; min / max = the first
sample, then x < acc ? x : acc and x > acc ? x : acc (one elementwise IEEE operation per sample and element, on the tensors where
they lie; no np.sum or torch.sum, which add pairwise); mean = that sum / n, divided by numpy on the CPU; counts = the number of
samples with x > threshold / x < threshold; a window without a sample holds 0 for sum and counts and NaN otherwise.  A wind speed is
numpy's sqrt(u * u + v * v) of the taped u and v.  Which samples belong to which window comes from the arbiter's tape_steps() and
from spd_wintape_plan, which tests/test_wintape_cpu.py pins -- not from Python's calendar.  Every comparison is BITWISE: an fp64
ring equals the arbiter, an fp32 ring its .float().

A member's trajectory does not depend on how many members its model has or on the launch plan, so one twin of 64 members serves
every fp64 case and one twin of 8 members the fp32-storage case."""
from datetime import datetime

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIGMA = ("u_grid", "v_grid", "t_grid", "q_grid", "phi_grid", "ps_grid", "precnv", "precls")
PLEV = ("u_plev", "v_plev", "t_plev", "q_plev", "z_plev", "mslp")
WSPD = {"wspd_grid": ("u_grid", "v_grid"), "wspd_plev": ("u_plev", "v_plev")}
NAMES = SIGMA + PLEV + tuple(WSPD)
OPS = ("sum", "mean", "min", "max", "count_above", "count_below")
LEVELS = [1000.0, 850.0, 500.0, 200.0, 10.0]  # hPa, as tests/test_tape_gpu.py
EVERY, SAMPLE_EVERY = 12, 3
CALLS = (5, 1, 7, 12, 3, 20)  # 48 steps, 4 windows of 4 samples, most closes and samples inside calls
TOTAL = sum(CALLS)
STATE = ("vor", "div", "t", "tr", "ps")
START = (1982, 1, 1, 0, 0)


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


def perturbed(spectral, bc, M, fp32=False, options=(), levels=LEVELS, start=START, months=1):
    """tests/test_tape_gpu.py: perturbed, with the start date and the number of SST-anomaly months as arguments"""
    import torch
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, M)
    if months > 1:
        model.init_sst_anom(months)
    model.set_bc(bc, start_date=start)
    for name, value in options:
        model.set_option(name, value)
    if fp32:
        model.set_physics_precision(True)
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng(i).normal(0.0, 0.01, (96, 48, 8)).transpose(2, 1, 0) for i in range(M)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()
    for n in SIGMA:  # (every view tests/test_tape_gpu.py takes is taken here, on every model alike: taking a view drops derived state)
        model.device_view(n)
    if levels:
        model.plev_configure(levels)
    return model


def step(model, n, checked=False):
    if checked:
        failed, _ = model.run_checked(n)
        assert (failed == -1).all()
    else:
        model.run(n)


def taped(names):
    """the catalogue names an fp64 tape must hold to restate `names`"""
    out = []
    for n in names:
        for t in WSPD.get(n, (n,)):
            if t not in out:
                out.append(t)
    return out


def arbiter(spectral, bc, M, names, sample_every, total, **kw):
    """{name: fp64 tensor [M][samples][levels][48][96] on the device} from the twin's fp64 tape, the step of every sample, and the
    spectral state after `total` steps"""
    import torch
    model = perturbed(spectral, bc, M, **kw)
    samples = total // sample_every
    model.tape_configure(taped(names), sample_every, samples, dtype="float64")
    model.run(total)
    assert model.tape_info["taken"] == samples
    series = {n: model.tape(n) for n in taped(names)}
    for n, (u, v) in WSPD.items():
        if n in names:
            a, b = series[u].cpu().numpy(), series[v].cpu().numpy()
            series[n] = torch.from_numpy(np.sqrt(a * a + b * b)).to(series[u].device)
    steps = model.tape_steps().tolist()
    torch.cuda.synchronize()
    state = {n: [model.get(n, i) for i in range(M)] for n in STATE}
    model.close()
    return {n: series[n] for n in names}, steps, state


def thresholds_of(series):
    """per name a value that splits the field: the median of the series, or its mean where nothing lies below or above the median
    (precipitation: zero at most points, and everywhere in the first steps after the start from rest)"""
    out = {}
    for n, x in series.items():
        t = float(x.flatten().median())
        if not bool((x < t).any()) or not bool((x > t).any()):
            t = float(x.mean())
        assert bool((x < t).any()) and bool((x > t).any()), n
        out[n] = t
    return out


def plan_rows(start, step0, nsteps, window, sample_every):
    import pyspeedy_amd
    return pyspeedy_amd.wintape_plan(start, step0, nsteps, window, sample_every).tolist()


def windows_of(rows, step0, sample_steps, sample_every):
    """per closed window of the plan the indices into the arbiter's samples that belong to it"""
    out, prev = [], step0
    for row in rows:
        idx = [i for i, s in enumerate(sample_steps) if prev < s <= row[0] and s % sample_every == 0]
        assert len(idx) == row[6], (row, idx)
        out.append(idx)
        prev = row[0]
    return out


def reduce_windows(series, windows, thresholds, entries=None, members=None):
    """{(name, op): fp64 tensor [M][windows][levels][48][96]} by the explicit loop in sample order"""
    import torch
    out = {}
    sl = slice(None) if members is None else slice(0, members)
    for name, x in series.items():
        wanted = [op for op in OPS if entries is None or (name, op) in entries]
        if not wanted:
            continue
        x = x[sl]
        thr = thresholds.get(name, 0.0)
        cols = {op: [] for op in OPS}
        for idx in windows:
            if not idx:
                zero, nan = torch.zeros_like(x[:, 0]), torch.full_like(x[:, 0], float("nan"))
                for op in OPS:
                    cols[op].append(zero if op in ("sum", "count_above", "count_below") else nan)
                continue
            first = x[:, idx[0]]
            s, lo, hi = first.clone(), first.clone(), first.clone()
            above, below = (first > thr).double(), (first < thr).double()
            for k in idx[1:]:  # in sample order
                v = x[:, k]
                s = s + v
                lo = torch.where(v < lo, v, lo)
                hi = torch.where(v > hi, v, hi)
                above = above + (v > thr).double()
                below = below + (v < thr).double()
            cols["sum"].append(s)
            cols["mean"].append(torch.from_numpy(s.cpu().numpy() / np.float64(len(idx))).to(s.device))  # one IEEE division
            cols["min"].append(lo)
            cols["max"].append(hi)
            cols["count_above"].append(above)
            cols["count_below"].append(below)
        for op in wanted:
            out[(name, op)] = torch.stack(cols[op], dim=1)
    return out


def entries_of(pairs, thresholds):
    return [(n, op, thresholds[n]) if op.startswith("count") else (n, op) for n, op in pairs]


ALL = tuple((n, op) for n in NAMES for op in OPS)


def assert_bitwise(got, ref, what):
    import torch
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if not torch.equal(got, ref):
        bad = got != ref
        raise AssertionError("%s: %d of %d values differ, max |diff| %.3e" % (
            what, int(bad.sum()), bad.numel(), float((got.double() - ref.double()).abs().max())))


def reference(spectral, bc, M, fp32=False):
    series, steps, state = arbiter(spectral, bc, M, NAMES, SAMPLE_EVERY, TOTAL, fp32=fp32)
    assert steps == list(range(SAMPLE_EVERY, TOTAL + 1, SAMPLE_EVERY))
    thresholds = thresholds_of(series)
    rows = plan_rows(START, 0, TOTAL, EVERY, SAMPLE_EVERY)
    assert [r[0] for r in rows] == [12, 24, 36, 48] and [r[6] for r in rows] == [4] * 4
    ref = reduce_windows(series, windows_of(rows, 0, steps, SAMPLE_EVERY), thresholds)
    return dict(series=series, steps=steps, state=state, thresholds=thresholds, rows=rows, ref=ref)


@pytest.fixture(scope="module")
def twin64(spectral, bc):
    return reference(spectral, bc, 64)


def test_the_arbiter_is_not_empty(twin64):
    """On the arbiter's own data, per name: inside at least one window, at some point, max > min and sum != n * last sample, and
    both counts lie strictly between 0 and n somewhere.  A recorder that kept only the last sample would otherwise pass."""
    ref, series = twin64["ref"], twin64["series"]
    last = [3, 7, 11, 15]  # the last sample of each window
    for name in NAMES:
        spread = ref[(name, "max")] > ref[(name, "min")]
        differs = ref[(name, "sum")] != 4.0 * series[name][:, last]
        both = spread & differs
        print("%-9s points that vary inside a window: %d of %d" % (name, int(both.sum()), both.numel()))
        assert bool(both.any()), name
        for op in ("count_above", "count_below"):
            c = ref[(name, op)]
            assert bool(((c >= 0) & (c <= 4) & (c == c.round())).all()), (name, op)
            assert bool((c > 0).any()) and bool((c < 4).any()), (name, op)


PLANS = {
    "serial_8": dict(M=8),
    "two_groups_64": dict(M=64),
    "rounds_32": dict(M=32, options=(("block_members", 4),), checked=True),
    "fp32_storage_8": dict(M=8, fp32=True),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_windows_equal_the_reduced_tape(spectral, bc, twin64, plan):
    """All sixteen names under all six ops at five levels, 4 windows of 12 steps with a sample every 3 over calls of 5, 1, 7, 12, 3
    and 20 steps: the fp64 ring is bitwise the arbiter's reduction and the fp32 ring its .float(), rows and counts are the plan's,
    and the recording model's spectral state after step 48 is bitwise the twin's -- serial, with two member groups, in rounds of
    block_members (checked calls), and with fp32 physics storage (precnv / precls stored as float)."""
    import torch
    p = PLANS[plan]
    M, options, fp32, checked = p["M"], p.get("options", ()), p.get("fp32", False), p.get("checked", False)
    twin = reference(spectral, bc, M, fp32=True) if fp32 else twin64
    entries = entries_of(ALL, twin["thresholds"])
    for dtype, torch_dtype in (("float64", torch.float64), ("float32", torch.float32)):
        model = perturbed(spectral, bc, M, fp32, options)
        model.wintape_configure(entries, EVERY, 4, sample_every=SAMPLE_EVERY, dtype=dtype)
        cfg = model.config()
        if plan == "serial_8":
            assert cfg["chunks"] == 1 and cfg["rounds"] == 1
        if plan == "two_groups_64":
            assert cfg["chunks"] == 2 and cfg["rounds"] == 1
        if plan == "rounds_32":
            assert cfg["rounds"] > 1
        if plan == "fp32_storage_8":
            assert cfg["physics_storage32"] and model.device_view("precnv").dtype == torch.float32
        for n in CALLS:
            step(model, n, checked)
        assert model.current_step == TOTAL
        assert model.wintape_info == dict(taken=4, held=4, capacity=4, window=EVERY, sample_every=SAMPLE_EVERY, dtype=dtype)
        assert model._wintape_rows().tolist() == twin["rows"]
        samples, steps = model.wintape_counts()
        assert samples.tolist() == [4] * 4 and steps.tolist() == [12] * 4 and model.wintape_steps().tolist() == [12, 24, 36, 48]
        for name, op in ALL:
            got = model.wintape(name, op)
            assert_bitwise(got, twin["ref"][(name, op)][:M].to(torch_dtype), "%s %s %s %s" % (plan, dtype, name, op))
        for n, per_member in twin["state"].items():
            for i in range(M):
                assert np.array_equal(model.get(n, i), per_member[i]), (plan, dtype, n, i)
        model.close()


def test_calendar_windows(spectral, bc):
    """2 members from 1982-01-31 12:00, ps_grid and mslp, a sample every 9 steps.  MONTH over 1062 steps in calls of 18, 500, 508
    and 36: the windows of the 12 hours of January left and of the 28-day February, 2 and 112 samples, bitwise.  DAY with a sample
    every 36 steps over 100 steps: three windows, the first without a sample -- sum and counts 0, mean, min and max NaN."""
    import torch
    start, M = (1982, 1, 31, 12, 0), 2
    names = ("ps_grid", "mslp")
    pairs = tuple((n, op) for n in names for op in OPS)
    series, sample_steps, state = arbiter(spectral, bc, M, names, 9, 1062, start=start, months=4)
    thresholds = thresholds_of(series)
    entries = entries_of(pairs, thresholds)
    # months
    rows = plan_rows(start, 0, 1062, "month", 9)
    assert rows == [[18, 1982, 2, 1, 0, 0, 2, 18], [1026, 1982, 3, 1, 0, 0, 112, 1008]]
    ref = reduce_windows(series, windows_of(rows, 0, sample_steps, 9), thresholds)
    model = perturbed(spectral, bc, M, start=start, months=4)
    model.wintape_configure(entries, "month", 4, sample_every=9, dtype="float64")
    for n in (18, 500, 508, 36):
        model.run(n)
    assert model.wintape_info == dict(taken=2, held=2, capacity=4, window="month", sample_every=9, dtype="float64")
    assert model._wintape_rows().tolist() == rows
    assert model.wintape_times() == [datetime(1982, 2, 1), datetime(1982, 3, 1)]
    samples, steps = model.wintape_counts()
    assert samples.tolist() == [2, 112] and steps.tolist() == [18, 1008]
    for name, op in pairs:
        assert_bitwise(model.wintape(name, op), ref[(name, op)], "month %s %s" % (name, op))
    assert float(ref[("ps_grid", "count_below")].max()) > 4.0  # (more than a few samples: the February window)
    for n, per_member in state.items():
        for i in range(M):
            assert np.array_equal(model.get(n, i), per_member[i]), ("month", n, i)
    model.close()
    # days, a sample every 36 steps: the arbiter's samples at steps 36 and 72
    rows = plan_rows(start, 0, 100, "day", 36)
    assert [r[0] for r in rows] == [18, 54, 90] and [r[6] for r in rows] == [0, 1, 1]
    windows = windows_of(rows, 0, sample_steps, 36)
    assert windows == [[], [3], [7]]
    ref = reduce_windows(series, windows, thresholds)
    model = perturbed(spectral, bc, M, start=start, months=4)
    model.wintape_configure(entries, "day", 3, sample_every=36, dtype="float32")
    model.run(100)
    assert model._wintape_rows().tolist() == rows
    samples, steps = model.wintape_counts()
    assert samples.tolist() == [0, 1, 1] and steps.tolist() == [18, 36, 36]
    for name, op in pairs:
        got = model.wintape(name, op)
        assert got.dtype == torch.float32
        if op in ("sum", "count_above", "count_below"):
            assert bool((got[:, 0] == 0).all()), (name, op)
        else:
            assert bool(torch.isnan(got[:, 0]).all()), (name, op)
        assert not bool(torch.isnan(got[:, 1:]).any())
        assert_bitwise(got[:, 1:], ref[(name, op)][:, 1:].float(), "day %s %s" % (name, op))
    model.close()


LIFE = (("t_grid", "mean"), ("wspd_grid", "max"), ("ps_grid", "min"), ("precnv", "sum"), ("t_grid", "count_below"), ("mslp", "count_above"))


def test_a_recorder_configured_after_two_steps_reset_and_the_ring(spectral, bc, twin64):
    """The first window after _configure starts at the model's current step; _reset in mid-window drops the open window's samples;
    the ring keeps the last `capacity` windows and _times follows it; reads of sub-ranges give the matching slices."""
    import torch
    M = 2
    series = {n: twin64["series"][n] for n in {n for n, _ in LIFE}}
    thresholds, sample_steps = twin64["thresholds"], twin64["steps"]
    entries = entries_of(LIFE, thresholds)
    model = perturbed(spectral, bc, M)
    model.run(2)
    model.wintape_configure(entries, EVERY, 3, sample_every=SAMPLE_EVERY, dtype="float64")
    assert model.wintape_info == dict(taken=0, held=0, capacity=3, window=EVERY, sample_every=SAMPLE_EVERY, dtype="float64")
    assert model.wintape("t_grid", "mean").shape == (M, 0, 8, 48, 96) and model.wintape_steps().tolist() == []
    for n in (3, 1, 7, 12, 3):  # to step 28
        model.run(n)
    rows = plan_rows((1982, 1, 1, 1, 20), 2, 26, EVERY, SAMPLE_EVERY)
    assert [r[0] for r in rows] == [12, 24] and [r[6] for r in rows] == [4, 4] and [r[7] for r in rows] == [10, 12]
    assert model._wintape_rows().tolist() == rows
    ref = reduce_windows(series, windows_of(rows, 2, sample_steps, SAMPLE_EVERY), thresholds, LIFE, M)
    for name, op in LIFE:
        assert_bitwise(model.wintape(name, op), ref[(name, op)], "short first window: %s %s" % (name, op))
    model.wintape_reset()  # at step 28: the open window's sample of step 27 is dropped, the next window holds steps 29 ... 36
    assert model.wintape_info["taken"] == 0
    model.run(20)
    samples, steps = model.wintape_counts()
    assert model.wintape_steps().tolist() == [36, 48] and samples.tolist() == [3, 4] and steps.tolist() == [8, 12]
    ref = reduce_windows(series, [[9, 10, 11], [12, 13, 14, 15]], thresholds, LIFE, M)
    for name, op in LIFE:
        assert_bitwise(model.wintape(name, op), ref[(name, op)], "after reset: %s %s" % (name, op))
    model.close()
    # capacity 2 with 4 windows taken, fp32
    model = perturbed(spectral, bc, M)
    model.wintape_configure(entries, EVERY, 2, sample_every=SAMPLE_EVERY)
    for n in CALLS:
        model.run(n)
    assert model.wintape_info == dict(taken=4, held=2, capacity=2, window=EVERY, sample_every=SAMPLE_EVERY, dtype="float32")
    assert model._wintape_rows().tolist() == twin64["rows"][2:]
    assert model.wintape_times() == [datetime(1982, 1, 2), datetime(1982, 1, 2, 8, 0)]
    one = np.zeros((1, 8), dtype=np.int32)
    assert model._lib.spd_model_wintape_times(model._m, one.ctypes.data_as(C.POINTER(C.c_int32)), 1) == 1  # (the oldest held)
    assert one.tolist() == [[36, 1982, 1, 2, 0, 0, 4, 12]]
    for name, op in LIFE:
        whole = model.wintape(name, op)
        assert_bitwise(whole, twin64["ref"][(name, op)][:M, 2:4].float(), "ring: %s %s" % (name, op))
        halves = torch.cat([model.wintape(name, op, t0=0, nt=1), model.wintape(name, op, t0=1, nt=1)], dim=1)
        assert_bitwise(halves, whole, name + " in two parts")
        assert_bitwise(model.wintape(name, op, first=1, count=1, t0=1, nt=1), whole[1:2, 1:2], name + " member 1, window 1")
    buf = torch.empty(8, dtype=torch.float32, device=model.sp.device)
    assert model._lib.spd_model_wintape_read(model._m, b"ps_grid", 2, 0, 2, 0, 2, buf.data_ptr(), 32, None) == -3  # SPD_E_SIZE
    model.close()


def test_reconfigure_off_checked_calls_init_and_validity(spectral, bc, twin64):
    """Reconfiguring with other entries and another window; _configure with 0 entries, after which calls fail with their reason;
    configuration, reset and reads are refused while a checked call is in flight; a checked call that reports a failed range check
    makes reads fail, naming member and step, until the next reset; spd_model_init and a step counter set by hand start a window."""
    from pyspeedy_amd._lib import SpeedyHipError
    M = 2
    thresholds, sample_steps = twin64["thresholds"], twin64["steps"]
    model = perturbed(spectral, bc, M)
    with pytest.raises(SpeedyHipError, match="no window tape configured"):
        model.wintape_info
    model.wintape_configure([("q_grid", "max")], 5, 2, dtype="float64")
    model.run(12)
    assert model.wintape_steps().tolist() == [5, 10]
    second = (("z_plev", "mean"), ("wspd_plev", "min"), ("precls", "max"))
    model.wintape_configure(second, EVERY, 3, sample_every=SAMPLE_EVERY, dtype="float64")  # at step 12
    assert model.wintape_info["taken"] == 0
    model.run(24)
    rows = plan_rows((1982, 1, 1, 8, 0), 12, 24, EVERY, SAMPLE_EVERY)
    assert model._wintape_rows().tolist() == rows and [r[0] for r in rows] == [24, 36]
    series = {n: twin64["series"][n] for n in ("z_plev", "wspd_plev", "precls")}
    ref = reduce_windows(series, windows_of(rows, 12, sample_steps, SAMPLE_EVERY), thresholds, second, M)
    for name, op in second:
        assert_bitwise(model.wintape(name, op), ref[(name, op)], "reconfigured: %s %s" % (name, op))
    with pytest.raises(SpeedyHipError, match="not among the configured entries"):
        model.wintape("q_grid", "max")
    with pytest.raises(SpeedyHipError, match="not among the configured entries"):
        model.wintape("z_plev", "max")
    with pytest.raises(SpeedyHipError, match="window range out of bounds"):
        model.wintape("z_plev", "mean", t0=1, nt=2)
    with pytest.raises(SpeedyHipError, match="member range out of bounds"):
        model.wintape("z_plev", "mean", first=1, count=2)
    with pytest.raises(ValueError, match="op must be"):
        model.wintape("z_plev", "median")
    with pytest.raises(ValueError, match="needs a threshold"):
        model.wintape_configure([("t_grid", "count_below")], "day", 2)
    with pytest.raises(ValueError, match="window must be"):
        model.wintape_configure([("t_grid", "mean")], "week", 2)
    with pytest.raises(SpeedyHipError, match="the window tape holds a pressure-level variable"):
        model.plev_configure([500.0])
    # off
    model.wintape_configure([], "day", 1)
    for call in (lambda: model.wintape("z_plev", "mean"), model.wintape_reset, model.wintape_steps):
        with pytest.raises(SpeedyHipError, match="no window tape configured"):
            call()
    model.plev_configure([500.0])
    model.run(3)
    # checked calls
    model.wintape_configure([("ps_grid", "mean")], 3, 2, dtype="float64")  # at step 39
    stream = model._stream()
    assert model._lib.spd_model_step_checked_begin(model._m, 4, stream) == 0
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.wintape("ps_grid", "mean")
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.wintape_configure([("ps_grid", "mean")], 3, 2)
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.wintape_reset()
    failed = np.zeros(M, dtype=np.int32)
    assert model._lib.spd_model_step_checked_end(model._m, failed.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    assert failed.tolist() == [-1, -1] and model.wintape_steps().tolist() == [42]
    # a member out of range: global-mean temperature of 500 K (diagnostics.f90:57-66), as tests/test_tape_gpu.py
    t = model.get("t", 1)
    t[0, 0, :, :] = 500.0 * np.sqrt(2.0)
    model.set("t", t, member=1)
    failed, _ = model.run_checked(3)
    assert failed.tolist() == [-1, 0]
    with pytest.raises(SpeedyHipError, match="invalid until spd_model_wintape_reset: member 1 failed the range check at step 0"):
        model.wintape("ps_grid", "mean")
    assert model.wintape_info["taken"] == 2  # (the count is still told)
    model.wintape_reset()
    assert model.wintape("ps_grid", "mean").shape == (M, 0, 48, 96)
    # spd_model_init: an empty ring and a window from step 0
    model.init(START)
    model.run(7)
    samples, steps = model.wintape_counts()
    assert model.wintape_steps().tolist() == [3, 6] and samples.tolist() == [3, 3] and steps.tolist() == [3, 3]
    # the step counter set by hand in mid-window (at step 7, to 100): the open window does not continue
    model.mark_initialized(100, (1982, 3, 1, 0, 0))
    model.run(3)
    samples, steps = model.wintape_counts()
    assert model.wintape_steps().tolist() == [6, 102] and samples.tolist() == [3, 2] and steps.tolist() == [3, 2]
    assert model.wintape_times()[1] == datetime(1982, 3, 1, 1, 20)
    model.init(START)
    assert model.wintape_info["taken"] == 0 and model.wintape_info["capacity"] == 2
    model.close()


def test_the_recorders_are_independent(spectral, bc, twin64):
    """The window tape gives bitwise the same with the tape and the accumulation tape on beside it as alone, they give the same as
    without it, and the final state -- every registry variable -- is bitwise that of a run with none of them."""
    import torch
    M = 3
    pairs = (("t_grid", "mean"), ("precnv", "max"), ("wspd_plev", "max"), ("mslp", "min"), ("q_grid", "count_above"))
    entries = entries_of(pairs, twin64["thresholds"])
    acc = (("precnv", "sum"), ("olr", "mean"))
    runs = {}
    for key, with_win, with_others in (("none", False, False), ("win", True, False), ("others", False, True), ("all", True, True)):
        model = perturbed(spectral, bc, M)
        if with_others:
            model.tape_configure(["precnv", "t_grid", "u_plev"], 3, 16, dtype="float64")
            model.acctape_configure(acc, 4, 12, dtype="float64")
        if with_win:
            model.wintape_configure(entries, EVERY, 4, sample_every=SAMPLE_EVERY, dtype="float64")
        for n in CALLS:
            model.run(n)
        out = {"state": {n: [model.get(n, i) for i in range(M)] for n in model.variables() if n not in ("lon", "lat", "lev")}}
        if with_others:
            assert model.tape_info["taken"] == 16 and model.acctape_info["taken"] == 12
            out["tape"] = {n: model.tape(n).clone() for n in ("precnv", "t_grid", "u_plev")}
            out["acc"] = {e: model.acctape(*e).clone() for e in acc}
        if with_win:
            assert model.wintape_info["taken"] == 4
            out["win"] = {e: model.wintape(*e).clone() for e in pairs}
        torch.cuda.synchronize()
        runs[key] = out
        model.close()
    for e in pairs:
        assert_bitwise(runs["all"]["win"][e], runs["win"]["win"][e], "beside the others: %s %s" % e)
        assert_bitwise(runs["win"]["win"][e], twin64["ref"][e][:M], "alone: %s %s" % e)
    for n in ("precnv", "t_grid", "u_plev"):
        assert_bitwise(runs["all"]["tape"][n], runs["others"]["tape"][n], "tape of " + n)
    for e in acc:
        assert_bitwise(runs["all"]["acc"][e], runs["others"]["acc"][e], "accumulation tape of %s %s" % e)
    for key in ("win", "others", "all"):
        for n, per_member in runs["none"]["state"].items():
            for a, b in zip(per_member, runs[key]["state"][n]):
                assert np.array_equal(a, b), (key, n)


def test_all_six_recorders_together_in_rounds_with_rings_that_wrap(spectral, bc):
    """Statistics, tape, spectra, ensemble tape, accumulation tape and window tape on at once, in ONE checked call of 13 steps that
    is issued as five rounds of 2, 2, 2, 2 and 1 members (9 members, two member groups, block_members 1: the last round leaves a
    group empty), into rings of two slots that wrap inside the call (the ensemble tape takes six samples and folds the last two
    only).  Everything a recorder hands out -- its info, steps, times, counts and every tensor -- equals what it hands out when it
    is the only one on in the same plan, and the final state, every registry variable, is bitwise that of a run with none."""
    import torch
    M, steps = 9, 13
    fields = ("t_grid", "precnv")
    names = ("ke_rot_spectrum", "lnps_mean")
    acc = (("precnv", "sum"), ("olr", "mean"))
    win = (("t_grid", "mean"), ("precnv", "max"), ("wspd_grid", "max"))
    configure = {
        "stats": lambda m: m.stats_configure(fields, 2, variance=True),
        "tape": lambda m: m.tape_configure(fields, 3, 2, dtype="float64"),
        "spectra": lambda m: m.spectra_configure(names, 2, 2),
        "enstape": lambda m: m.enstape_configure(fields, 2, 2),
        "acctape": lambda m: m.acctape_configure(acc, 3, 2, dtype="float64"),
        "wintape": lambda m: m.wintape_configure(win, 2, 2, sample_every=1, dtype="float64"),
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
    }
    taken = {"tape": 4, "spectra": 6, "enstape": 6, "acctape": 4, "wintape": 6}  # 13 steps from step 0, every 3 or 2

    def run(on):
        model = perturbed(spectral, bc, M, options=(("member_groups", 2), ("block_members", 1)), levels=None)
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

    def assert_same(got, ref, what):
        if torch.is_tensor(ref):
            assert_bitwise(got, ref, what)
        elif isinstance(ref, dict):
            assert got.keys() == ref.keys(), what
            for k in ref:
                assert_same(got[k], ref[k], "%s, %s" % (what, k))
        elif isinstance(ref, tuple):
            assert len(got) == len(ref), what
            for k, (a, b) in enumerate(zip(got, ref)):
                assert_same(a, b, "%s, %d" % (what, k))
        else:
            assert got == ref, (what, got, ref)

    together, none = run(tuple(configure)), run(())
    assert together["stats"]["samples"] == 6
    for key, n in taken.items():  # (every ring has wrapped)
        assert together[key]["info"]["taken"] == n and together[key]["info"]["held"] == 2 and len(together[key]["steps"]) == 2, key
    for key in configure:
        assert_same(together[key], run((key,))[key], key + " beside the others")
    for n, per_member in none["state"].items():
        for i, (a, b) in enumerate(zip(together["state"][n], per_member)):
            assert np.array_equal(a, b), (n, i)


def test_shapes_dtypes_device_and_levels(spectral, bc):
    """wintape() follows the tape's shape conventions, in the ring's dtype, on the model's device; pressure-level names (the wind
    speed at levels among them) are refused before levels are configured."""
    import torch
    from pyspeedy_amd._lib import SpeedyHipError
    M = 2
    model = perturbed(spectral, bc, M, levels=None)
    for name in PLEV + ("wspd_plev",):
        with pytest.raises(SpeedyHipError, match="'%s' needs target levels" % name):
            model.wintape_configure([("t_grid", "mean"), (name, "mean")], 4, 2)
    with pytest.raises(SpeedyHipError, match="no window tape configured"):
        model.wintape_info
    model.plev_configure([850.0, 500.0, 250.0])
    pairs = (("t_grid", "mean"), ("ps_grid", "max"), ("precls", "sum"), ("wspd_grid", "max"), ("z_plev", "min"), ("wspd_plev", "mean"),
             ("mslp", "count_above"))
    shapes = {"t_grid": (8, 48, 96), "ps_grid": (48, 96), "precls": (48, 96), "wspd_grid": (8, 48, 96), "z_plev": (3, 48, 96),
              "wspd_plev": (3, 48, 96), "mslp": (48, 96)}
    for dtype, torch_dtype in (("float32", torch.float32), ("float64", torch.float64), (torch.float32, torch.float32)):
        model.wintape_configure([(n, op, 101000.0) if op.startswith("count") else (n, op) for n, op in pairs], 2, 3, dtype=dtype)
        model.run(4)
        for name, op in pairs:
            got = model.wintape(name, op)
            assert got.shape == (M, 2) + shapes[name] and got.dtype == torch_dtype and got.device == model.device_view("t_grid").device
            assert got.is_contiguous() and bool(torch.isfinite(got).all())
            assert model.wintape(name, op, first=1, t0=1).shape == (1, 1) + shapes[name]
        wind = model.wintape("wspd_grid", "max")
        assert float(wind.min()) >= 0.0 and float(wind.max()) > 1.0
    with pytest.raises(ValueError, match="dtype must be"):
        model.wintape_configure([("t_grid", "mean")], 2, 3, dtype="float16")
    model.close()
