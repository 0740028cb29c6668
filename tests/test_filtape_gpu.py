"""GPU tier: window means, covariances and last values of time-filtered fields recorded on the device (spd_model_filtape_*,
EnsembleModel.filtape_*).

The arbiter is existing code plus numpy: a twin model built by `perturbed` of tests/test_wintape_gpu.py (t_grid += N(0, 0.01 K),
seed = member id) that holds an fp64 TAPE of the names among the entries with every = the recorder's sample_every.  The taped planes
are filtered and reduced on the CPU by tests/filtape_reference.py in sample order -- the numpy restatement that
tests/test_filtape_cpu.py holds to a loop over Python floats and to the library's host compile of the kernel's routines.  Which
samples belong to which window comes from the arbiter's tape_steps() and from spd_wintape_plan; which of them are counted from the
filter sample number and the spin-up.  Every comparison is on BIT PATTERNS: an fp64 ring equals the arbiter, an fp32 ring its
.astype(float32).

A member's trajectory does not depend on how many members its model has or on the launch plan, so one twin of 64 members serves
every fp64 case and one twin of 8 members the fp32-storage case."""
import ctypes as C

import numpy as np
import pytest

import crowd_cases as cc
import filtape_reference as ref
from test_wintape_gpu import LEVELS, START, perturbed, plan_rows, step

pytestmark = pytest.mark.gpu

EVERY, SAMPLE_EVERY, SPINUP = 12, 3, 5
CALLS = (5, 1, 7, 12, 3, 20)  # 48 steps: the spin-up ends (sample 6, step 18) and the windows close inside calls
TOTAL = sum(CALLS)
STATE = ("vor", "div", "t", "tr", "ps")
LOW, BAND = 0, 1
# (name, level, filter, op[, name_b, level_b]): levels of pressure-level names in hPa
ENTRIES = (
    ("z_plev", 500.0, LOW, "mean"),
    ("z_plev", 500.0, BAND, "cov"),
    ("v_plev", 850.0, BAND, "cov", "t_plev", 850.0),
    ("mslp", 0, BAND, "last"),
    ("u_grid", 2, LOW, "cov", "precnv", 0),
    ("precnv", 0, BAND, "mean"),
    ("omega_plev", 500.0, BAND, "cov"),
)
E = len(ENTRIES)
TAPED = ("u_grid", "precnv", "v_plev", "t_plev", "z_plev", "mslp", "omega_plev")
ON_LEVELS = ("v_plev", "t_plev", "z_plev", "omega_plev")
OPS = {"mean": ref.MEAN, "cov": ref.COV, "last": ref.LAST}
PLANES = 9  # z500 under both filters, v850, t850, mslp, omega500 and precnv under the band-pass, u_grid 2 and precnv under the low-pass


def level_index(name, level):
    return LEVELS.index(level) if name in ON_LEVELS else int(level)


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


@pytest.fixture(scope="module")
def filters():
    """edges counted in samples: a one-section low-pass and a two-section band-pass"""
    import pyspeedy_amd
    low, band = pyspeedy_amd.butterworth_sections("lowpass", 2, 6.0, 1.0), pyspeedy_amd.butterworth_sections("bandpass", 2, (3.0, 8.0), 1.0)
    assert low.shape == (1, 5) and band.shape == (2, 5)
    return [low, band]


def twin(spectral, bc, M, total=TOTAL, sample_every=SAMPLE_EVERY, fp32=False, **kw):
    """dict(planes: {(name, level index): numpy [samples][M][48][96]} from the twin's fp64 tape, steps: the step of each sample,
    state: the spectral state after `total` steps)"""
    import torch
    model = perturbed(spectral, bc, M, fp32, **kw)
    samples = total // sample_every
    model.tape_configure(TAPED, sample_every, samples, dtype="float64")
    model.run(total)
    assert model.tape_info["taken"] == samples
    wanted = sorted({(e[0], level_index(e[0], e[1])) for e in ENTRIES} | {(e[4], level_index(e[4], e[5])) for e in ENTRIES if len(e) == 6})
    planes = {}
    for name in TAPED:
        x = model.tape(name)
        for n, k in wanted:
            if n == name:
                planes[(n, k)] = np.ascontiguousarray(np.moveaxis((x if x.dim() == 4 else x[:, :, k]).cpu().numpy(), 0, 1))
        del x
    steps = model.tape_steps().tolist()
    torch.cuda.synchronize()
    state = {n: [model.get(n, i) for i in range(M)] for n in STATE}
    model.close()
    return dict(planes=planes, steps=steps, state=state)


def reduce(tw, filters, rows, step0, spinup, M=None, first_sample=0, entries=ENTRIES):
    """the arbiter's rings: per entry numpy [M][windows][48][96].  The series starts at the twin's sample `first_sample`, which is
    filter sample 1; rows: the closed windows of the schedule, the first of which opened at step0."""
    windows = ref.counted_windows(rows, step0, tw["steps"][first_sample:], spinup)
    filtered = {}

    def y_of(name, level, f):
        key = (name, level_index(name, level), f)
        if key not in filtered:
            x = tw["planes"][key[:2]][first_sample:, :M]
            filtered[key] = ref.filter_series(filters[f], x)
        return filtered[key]

    out = []
    for e in entries:
        ya = y_of(e[0], e[1], e[2])
        yb = y_of(e[4], e[5], e[2]) if len(e) == 6 else ya
        out.append(np.ascontiguousarray(np.moveaxis(ref.reduce_windows(ya, yb, OPS[e[3]], windows), 0, 1)))
    return out, windows


def counted_rows(rows, windows):
    """the recorder's rows: the schedule's with the counted samples in column 6"""
    return [r[:6] + [len(w)] + r[7:] for r, w in zip(rows, windows)]


def assert_bits(got, expected, what):
    """got: a device tensor, expected: numpy of the same dtype; bit patterns, so that NaN and the sign of a zero count"""
    got = got.cpu().numpy()
    assert got.shape == expected.shape and got.dtype == expected.dtype, (what, got.shape, expected.shape, got.dtype, expected.dtype)
    as_int = np.uint64 if got.dtype == np.float64 else np.uint32
    a, b = got.view(as_int), expected.view(as_int)
    if not np.array_equal(a, b):
        where = tuple(np.argwhere(a != b)[0])
        raise AssertionError("%s: %d of %d values differ, first at %s: %r against %r" % (what, int((a != b).sum()), a.size, list(where), got[where],
                                                                                      expected[where]))


def reference(spectral, bc, filters, M, fp32=False):
    tw = twin(spectral, bc, M, fp32=fp32)
    assert tw["steps"] == list(range(SAMPLE_EVERY, TOTAL + 1, SAMPLE_EVERY))
    rows = plan_rows(START, 0, TOTAL, EVERY, SAMPLE_EVERY)
    rings, windows = reduce(tw, filters, rows, 0, SPINUP)
    assert windows == [[], [5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]]  # the first window empty, the second with three counted samples
    tw.update(rings=rings, rows=counted_rows(rows, windows))
    return tw


@pytest.fixture(scope="module")
def twin64(spectral, bc, filters):
    return reference(spectral, bc, filters, 64)


def test_the_arbiter_is_not_blind(twin64):
    """Per entry, on the arbiter alone: the values of some non-empty window are neither all equal nor all zero (precnv is zero at the
    start from rest: a field that stayed constant would let any recorder pass), the empty first window is NaN, and a covariance is
    not the square of a mean or a last value -- the filters and the ops do something."""
    for k, (entry, ring) in enumerate(zip(ENTRIES, twin64["rings"])):
        assert ring.shape == (64, 4, 48, 96) and np.isnan(ring[:, 0]).all() and np.isfinite(ring[:, 1:]).all(), entry
        alive = [w for w in (1, 2, 3) if np.ptp(ring[:, w]) > 0.0 and np.any(ring[:, w] != 0.0)]
        print("entry %d %r: windows whose values vary: %s; window 3 spans %.6g ... %.6g" % (k, entry, alive, ring[:, 3].min(), ring[:, 3].max()))
        assert alive, entry
        assert np.ptp(ring[:, 3]) > 0.0 and np.any(ring[:, 3] != 0.0), entry
    assert (twin64["rings"][1] >= 0.0)[:, 1:].all() and not (twin64["rings"][2][:, 1:] >= 0.0).all()  # a variance, and a flux of both signs
    # the band-passed mslp is a small part of mslp, the low-passed z500 close to z500
    assert np.abs(twin64["rings"][3][:, 1:]).max() < 5000.0 < np.abs(twin64["planes"][("mslp", 0)]).min()
    assert np.abs(twin64["rings"][0][:, 3] - twin64["planes"][("z_plev", 2)][15]).max() < 500.0 < twin64["planes"][("z_plev", 2)].min()


PLANS = {
    "serial_8": dict(M=8),
    "two_groups_64": dict(M=64),
    "rounds_32": dict(M=32, options=(("block_members", 4),), checked=True),
    "fp32_storage_8": dict(M=8, fp32=True),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_windows_equal_the_filtered_tape(spectral, bc, filters, twin64, plan):
    """Seven entries under two filters, 4 windows of 12 steps with a sample every 3 and a spin-up of 5 samples over calls of 5, 1, 7,
    12, 3 and 20 steps: the fp64 ring is bitwise the arbiter's and the fp32 ring its .astype(float32), rows and counts are the
    schedule's with the counted samples, and the recording model's spectral state after step 48 is bitwise the twin's -- serial, with
    two member groups, in rounds of block_members (checked calls), and with fp32 physics storage (precnv stored as float)."""
    import torch
    p = PLANS[plan]
    M, options, fp32, checked = p["M"], p.get("options", ()), p.get("fp32", False), p.get("checked", False)
    tw = reference(spectral, bc, filters, M, fp32=True) if fp32 else twin64
    for dtype, numpy_dtype in (("float64", np.float64), ("float32", np.float32)):
        model = perturbed(spectral, bc, M, fp32, options)
        model.filtape_configure(filters, ENTRIES, EVERY, 4, sample_every=SAMPLE_EVERY, spinup=SPINUP, dtype=dtype)
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
        assert model.filtape_info == dict(taken=4, held=4, capacity=4, window=EVERY, sample_every=SAMPLE_EVERY, spinup=SPINUP, dtype=dtype,
                                          filters=2, planes=PLANES, entries=E, filter_samples=16)
        assert model._filtape_rows().tolist() == tw["rows"]
        counted, steps = model.filtape_counts()
        assert counted.tolist() == [0, 3, 4, 4] and steps.tolist() == [12] * 4 and model.filtape_steps().tolist() == [12, 24, 36, 48]
        for k in range(E):
            got = model.filtape(k)
            assert bool(torch.isnan(got[:, 0]).all())
            assert_bits(got, tw["rings"][k][:M].astype(numpy_dtype), "%s %s entry %d %r" % (plan, dtype, k, ENTRIES[k]))
        for n, per_member in tw["state"].items():
            for i in range(M):
                assert np.array_equal(model.get(n, i), per_member[i]), (plan, dtype, n, i)
        model.close()


def test_day_windows(spectral, bc, filters):
    """SPD_WINDOW_DAY over 72 steps from 00:00 in calls of 30 and 42: two windows that close at midnight, 7 (12 less the spin-up) and
    12 counted samples; the ring of capacity 1 keeps the second."""
    M = 2
    tw = twin(spectral, bc, M, total=72)
    rows = plan_rows(START, 0, 72, "day", SAMPLE_EVERY)
    assert [r[0] for r in rows] == [36, 72]
    rings, windows = reduce(tw, filters, rows, 0, SPINUP)
    assert [len(w) for w in windows] == [7, 12]
    for capacity in (2, 1):
        model = perturbed(spectral, bc, M)
        model.filtape_configure(filters, ENTRIES, "day", capacity, sample_every=SAMPLE_EVERY, spinup=SPINUP, dtype="float64")
        model.run(30)
        model.run(42)
        assert model.filtape_info["window"] == "day" and model.filtape_info["taken"] == 2 and model.filtape_info["held"] == capacity
        assert model._filtape_rows().tolist() == counted_rows(rows, windows)[2 - capacity:]
        for k in range(E):
            assert_bits(model.filtape(k), rings[k][:, 2 - capacity:], "day windows, capacity %d, entry %d" % (capacity, k))
        model.close()


def test_reset_in_mid_run_restarts_the_filters(spectral, bc, filters, twin64):
    """filtape_reset() at step 20: the ring is empty, the next window starts there, and the sample of step 21 is filter sample 1 --
    the arbiter filters the twin's samples from that one on.  The spin-up of 2 then ends inside the first window."""
    M = 2
    model = perturbed(spectral, bc, M)
    model.filtape_configure(filters, ENTRIES, EVERY, 4, sample_every=SAMPLE_EVERY, spinup=2, dtype="float64")
    for n in (5, 1, 7, 7):
        model.run(n)
    assert model.filtape_info["taken"] == 1 and model.filtape_info["filter_samples"] == 6
    model.filtape_reset()
    assert model.filtape_info["taken"] == 0 and model.filtape_info["filter_samples"] == 0 and model.filtape(0).shape == (M, 0, 48, 96)
    for n in (5, 3, 20):
        model.run(n)
    rows = plan_rows((1982, 1, 1, 13, 20), 20, 28, EVERY, SAMPLE_EVERY)
    assert [r[0] for r in rows] == [24, 36, 48] and [r[7] for r in rows] == [4, 12, 12]
    rings, windows = reduce(twin64, filters, rows, 20, 2, M, first_sample=6)
    assert windows == [[], [2, 3, 4, 5], [6, 7, 8, 9]]
    assert model._filtape_rows().tolist() == counted_rows(rows, windows) and model.filtape_info["filter_samples"] == 10
    for k in range(E):
        assert_bits(model.filtape(k), rings[k], "after a reset, entry %d" % k)
    # the filters did restart: what a recorder that kept its state would hold differs
    kept, _ = reduce(twin64, filters, plan_rows(START, 0, TOTAL, EVERY, SAMPLE_EVERY), 0, 8, M)
    assert not np.array_equal(kept[1][:, 2:], rings[1][:, 1:])
    model.close()


def test_one_call_equals_single_steps_and_sub_ranges(spectral, bc, filters, twin64):
    """run(48) against 48 x run(1), both the arbiter's; reads of sub-ranges give the matching slices; SPD_E_SIZE for a small buffer."""
    import torch
    M = 3
    got = []
    for calls in ((TOTAL,), (1,) * TOTAL):
        model = perturbed(spectral, bc, M)
        model.filtape_configure(filters, ENTRIES, EVERY, 4, sample_every=SAMPLE_EVERY, spinup=SPINUP, dtype="float64")
        for n in calls:
            model.run(n)
        got.append([model.filtape(k).clone() for k in range(E)])
        assert model._filtape_rows().tolist() == twin64["rows"]
        if len(calls) == 1:
            whole = got[0][2]
            halves = torch.cat([model.filtape(2, t0=0, nt=2), model.filtape(2, t0=2, nt=2)], dim=1)
            assert torch.equal(halves[:, 1:], whole[:, 1:]) and bool(torch.isnan(halves[:, 0]).all())
            assert torch.equal(model.filtape(2, first=1, count=1, t0=3, nt=1), whole[1:2, 3:4])
            buf = torch.empty(8, dtype=torch.float64, device=model.sp.device)
            assert model._lib.spd_model_filtape_read(model._m, 0, 0, 1, 0, 1, buf.data_ptr(), 64, None) == -3  # SPD_E_SIZE
        model.close()
    for k in range(E):
        assert_bits(got[0][k], twin64["rings"][k][:M], "one call, entry %d" % k)
        assert_bits(got[1][k], twin64["rings"][k][:M], "single steps, entry %d" % k)


def test_the_run_does_not_change_and_off_is_off(spectral, bc, filters):
    """With the recorder on, every registry variable after the run is bitwise that of a run without it; filtape_off() in mid-run
    leaves a model whose state is that of one never configured, and whose calls fail with their reason."""
    from pyspeedy_amd._lib import SpeedyHipError
    M = 3
    runs = {}
    for key in ("never", "on", "off"):
        model = perturbed(spectral, bc, M)
        if key != "never":
            model.filtape_configure(filters, ENTRIES, EVERY, 4, sample_every=SAMPLE_EVERY, spinup=SPINUP)
        for i, n in enumerate(CALLS):
            if key == "off" and i == 3:
                model.filtape_off()
                assert model.filtape_entries == ()
            model.run(n)
        if key == "on":
            assert model.filtape_info["taken"] == 4
        else:
            for call in (lambda: model.filtape_info, lambda: model.filtape(0), model.filtape_reset, model.filtape_steps):
                with pytest.raises(SpeedyHipError, match="no filter tape configured"):
                    call()
        runs[key] = {n: [model.get(n, i) for i in range(M)] for n in model.variables() if n not in ("lon", "lat", "lev")}
        model.close()
    for key in ("on", "off"):
        for n, per_member in runs["never"].items():
            for a, b in zip(per_member, runs[key][n]):
                assert np.array_equal(a, b), (key, n)


def test_solo_against_crowd(spectral, bc, filters, twin64):
    """Configured together with a tape, the window tape, the projection tape and the track tape in one model and stepped through the
    same calls, the filter tape's ring is its solo run's (the arbiter's), and theirs are their solo runs'."""
    import torch
    M = 3
    weights = cc.weight_maps()
    track = (("mslp", 0, 0, "min", 0), ("t_grid", 7, 1, "max", 2))
    proj = tuple(e for e in cc.PROJTAPE if e[0] != "z_plev") + (("z_plev", 2, 0),)
    configure = {
        "tape": lambda m: m.tape_configure(["precnv", "t_grid", "z_plev"], 3, 16, dtype="float64"),
        "wintape": lambda m: m.wintape_configure(cc.WINTAPE, 6, 8, sample_every=2, dtype="float64"),
        "projtape": lambda m: m.projtape_configure(weights, proj, 2, 24),
        "tracktape": lambda m: m.tracktape_configure(weights[:2], track, 3, 16),
        "filtape": lambda m: m.filtape_configure(filters, ENTRIES, EVERY, 4, sample_every=SAMPLE_EVERY, spinup=SPINUP, dtype="float64"),
    }
    read = {
        "tape": lambda m: [m.tape(n).clone() for n in ("precnv", "t_grid", "z_plev")],
        "wintape": lambda m: [m.wintape(*e[:2]).clone() for e in cc.WINTAPE],
        "projtape": lambda m: [m.projtape().clone()],
        "tracktape": lambda m: [m.tracktape().clone()],
        "filtape": lambda m: [m.filtape(k).clone() for k in range(E)],
    }

    def run(on):
        model = perturbed(spectral, bc, M)
        for key in on:
            configure[key](model)
        for n in CALLS:
            model.run(n)
        out = {key: read[key](model) for key in on}
        torch.cuda.synchronize()
        model.close()
        return out

    crowd = run(tuple(configure))
    for key in configure:
        solo = crowd[key] if key == "filtape" else run((key,))[key]
        for k, (a, b) in enumerate(zip(crowd[key], solo)):
            same = (a == b) | (torch.isnan(a) & torch.isnan(b))
            assert a.shape == b.shape and bool(same.all()), (key, k)
    for k in range(E):
        assert_bits(crowd["filtape"][k], twin64["rings"][k][:M], "in the crowd, entry %d" % k)


def test_lifecycle_checked_calls_and_validity(spectral, bc, filters):
    """Configuration, reset, off and reads are refused while a checked call is in flight; spd_model_plev_configure is refused while
    an entry names a pressure-level plane; a level that is not configured is refused in Python; a checked call that reports a failed
    range check makes filtape() refuse, naming member and step, until the next reset; spd_model_init and a step counter set by hand
    restart the filters and the window."""
    from pyspeedy_amd._lib import SpeedyHipError
    M = 2
    model = perturbed(spectral, bc, M)
    with pytest.raises(SpeedyHipError, match="no filter tape configured"):
        model.filtape_info
    with pytest.raises(ValueError, match="not among the configured pressure levels"):
        model.filtape_configure(filters, [("z_plev", 300.0, 0, "mean")], 3, 2)
    with pytest.raises(ValueError, match="op must be"):
        model.filtape_configure(filters, [("t_grid", 0, 0, "median")], 3, 2)
    with pytest.raises(SpeedyHipError, match="filter 2 of entry 0"):
        model.filtape_configure(filters, [("t_grid", 0, 2, "mean")], 3, 2)
    model.filtape_configure(filters, [("ps_grid", 0, LOW, "mean"), ("z_plev", 500.0, BAND, "cov")], 3, 2, dtype="float64")
    assert model.filtape_entries == (("ps_grid", 0, 0, 0, "", 0), ("z_plev", 2, 1, 1, "", 0))
    with pytest.raises(SpeedyHipError, match="the filter tape holds a pressure-level variable"):
        model.plev_configure([500.0])
    with pytest.raises(SpeedyHipError, match="entry 2 is out of range"):
        model.filtape(2)
    stream = model._stream()
    assert model._lib.spd_model_step_checked_begin(model._m, 4, stream) == 0
    for call in (lambda: model.filtape(0), model.filtape_reset, model.filtape_off,
                 lambda: model.filtape_configure(filters, [("ps_grid", 0, LOW, "mean")], 3, 2)):
        with pytest.raises(SpeedyHipError, match="in flight"):
            call()
    failed = np.zeros(M, dtype=np.int32)
    assert model._lib.spd_model_step_checked_end(model._m, failed.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    assert failed.tolist() == [-1, -1] and model.filtape_steps().tolist() == [3] and model.filtape_info["filter_samples"] == 4
    # a member out of range: global-mean temperature of 500 K (diagnostics.f90:57-66), as tests/test_tape_gpu.py
    t = model.get("t", 1)
    t[0, 0, :, :] = 500.0 * np.sqrt(2.0)
    model.set("t", t, member=1)
    failed, _ = model.run_checked(3)
    assert failed.tolist() == [-1, 0]
    with pytest.raises(SpeedyHipError, match="invalid until spd_model_filtape_reset: member 1 failed the range check at step 0"):
        model.filtape(0)
    assert model.filtape_info["taken"] == 2  # (the count is still told)
    model.filtape_reset()
    assert model.filtape(0).shape == (M, 0, 48, 96)
    # spd_model_init: an empty ring, a window from step 0, filter sample 1 at the first step
    model.init(START)
    model.run(7)
    counted, steps = model.filtape_counts()
    assert model.filtape_steps().tolist() == [3, 6] and counted.tolist() == [3, 3] and steps.tolist() == [3, 3]
    assert model.filtape_info["filter_samples"] == 7
    # the step counter set by hand in mid-window (at step 7, to 100): neither the window nor the filters continue
    model.mark_initialized(100, (1982, 3, 1, 0, 0))
    model.run(3)
    counted, steps = model.filtape_counts()
    assert model.filtape_steps().tolist() == [6, 102] and counted.tolist() == [3, 2] and steps.tolist() == [3, 2]
    assert model.filtape_info["filter_samples"] == 3
    model.close()
