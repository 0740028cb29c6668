"""GPU tier: spectra by total wavenumber and global means of the spectral state, recorded on the device inside multi-step calls or
computed on the state as it stands (spd_model_spectra_*, EnsembleModel.spectra_* / spectrum).

Two arbiters.  The numbers: tests/spectra_reference.py (numpy fp64, written from the definition) on the state read back through
get().  The recording: the loop a user writes without it -- a twin model built by the same seeded perturbation as
tests/test_tape_gpu.py (t_grid += N(0, 0.01 K), seed = member id), stepped in calls of one step with spectrum() after each; every
comparison of a stored name with the twin is BITWISE."""
from datetime import datetime, timedelta

import ctypes as C

import numpy as np
import pytest

import spectra_reference as ref

pytestmark = pytest.mark.gpu

NAMES = ref.NAMES
DERIVED = ("ke_spectrum", "ke_mean", "ke_column")
STATE = ("vor", "div", "t", "tr", "ps")
M = 4
STEPS = 12


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


def perturbed(spectral, bc, members=M, options=()):
    import torch
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, members)
    model.set_bc(bc, start_date=(1982, 1, 1, 0, 0))
    for name, value in options:
        model.set_option(name, value)
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng(i).normal(0.0, 0.01, (96, 48, 8)).transpose(2, 1, 0) for i in range(members)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()
    return model


def registry(model):
    return {n: [model.get(n, i) for i in range(model.nmembers)] for n in model.variables() if n not in ("lon", "lat", "lev")}


@pytest.fixture(scope="module")
def twin(spectral, bc):
    """The hand-rolled loop: 4 members, 12 calls of one step, spectrum() after each -> ({name: [M][12][...] on the device}, the
    step counter and the date after each step, every registry variable after step 12)."""
    import torch
    model = perturbed(spectral, bc)
    series, steps, dates = {n: [] for n in NAMES + DERIVED}, [], []
    for _ in range(STEPS):
        model.run(1)
        for n, x in model.spectrum(NAMES + DERIVED).items():
            series[n].append(x.clone())
        steps.append(model.current_step)
        dates.append(datetime(*model.current_date))
    torch.cuda.synchronize()
    state = registry(model)
    model.close()
    return {n: torch.stack(v, dim=1) for n, v in series.items()}, steps, dates, state


def assert_same(got, want, what, name):
    """Bitwise for what the device stores.  The three derived names are torch sums over l (and the levels) of what was read, and torch
    may order a sum differently for another shape of tensor: at most 32 + 1 + 8 + 1 roundings of non-negative terms on each side,
    2 * 42 * 2^-53 = 9.3e-15, so within 1e-14 of the value."""
    import torch
    if name in DERIVED:
        assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
        assert torch.allclose(got, want, rtol=1e-14, atol=0.0), (what, float(((got - want).abs() / want).max()))
    else:
        assert_bitwise(got, want, what)


def assert_bitwise(got, want, what):
    import torch
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = got != want
        raise AssertionError("%s: %d of %d values differ, max |diff| %.3e" % (what, int(bad.sum()), bad.numel(),
                                                                              float((got - want).abs().max())))


def test_spectrum_against_the_arbiter(spectral, bc, golden_dir):
    """3 members after 36 steps, all names.  Against the arbiter on the state read back through get(): every bin within 1e-14 of
    its value (both sides sum at most 31 non-negative terms of a few roundings each: at most 2 (30 + 4) 2^-53 = 7.5e-15 apart),
    bins the arbiter leaves empty exactly 0, the three means bitwise.  The sample the device loop took at step 36 is bitwise the
    same."""
    import torch
    members = 3
    model = perturbed(spectral, bc, members)
    model.spectra_configure(NAMES, 36, 2)
    model.run(36)
    got = model.spectrum()
    assert tuple(got) == NAMES
    tables = np.load(golden_dir + "/tables.npz")  # (the reference's tables: nothing of the library under test)
    elm2 = tables["elm2"]
    worst = 0.0
    for i in range(members):
        state = {n: model.get(n, i)[..., 0] for n in STATE}  # time level 1
        want = ref.spectra(state["vor"], state["div"], state["t"], state["tr"], state["ps"], elm2)
        for n in NAMES:
            g, w = got[n][i].cpu().numpy(), want[n]
            assert g.shape == w.shape and g.dtype == np.float64, (n, g.shape, w.shape)
            if n.endswith("_mean"):
                assert np.array_equal(g, w), (n, i, g, w)
                continue
            assert not g[w == 0.0].any(), (n, i)
            rel = np.abs(g - w)[w != 0.0] / w[w != 0.0]
            worst = max(worst, float(rel.max()))
            assert (rel <= 1e-14).all(), (n, i, float(rel.max()))
            if n in ("ke_rot_spectrum", "t_spectrum"):
                assert (w[..., 1:31] > 0.0).all(), n  # (a real spectrum: every bin of the truncation holds something)
        assert not got["ke_rot_spectrum"][i, :, 0].any()  # (elm2 is 0 at l = 0)
    print("largest relative difference from the arbiter: %.2e" % worst)
    # the sample of the device loop at that step
    assert model.spectra_steps().tolist() == [36]
    for n in NAMES:
        assert_bitwise(model.spectra(n)[:, 0], got[n], "sample at step 36 of " + n)
    model.close()


def test_sample_against_the_export_on_the_device(spectral, bc, golden_dir, oracle):
    """The sum over l of both kinetic-energy spectra of the sample at step 36 against the Gaussian-weighted mean of
    (u_grid^2 + v_grid^2) / 2 after spectral2grid() at that step: within the 2e-4 of the CPU tier (tests/test_spectra_cpu.py) on
    every level but level 1.

    Level 1 cannot hold 2e-4 on this state, and the reason is the reference's quadrature, not the device: the CPU oracle alone (its
    vort2vel + spec2grid(kcos = 2) and Gaussian weights against the numpy arbiter, no device code) gives 2.6e-4 there at step 36,
    and swings between 6e-6 and 4.3e-4 over steps 12 ... 36 while the start from rest adjusts (the other levels: at most 1.8e-4).
    So the test runs that oracle comparison itself, on the state it reads back from the device, and level 1 must not exceed what the
    oracle gives for it -- and on EVERY level the device's difference must be the oracle's to within 1e-10: the export agrees with
    the oracle's transforms to 1e-12 of the largest value (the smoke test's parity), the kinetic energy is quadratic in them and
    the mean runs over 4608 points, so the two grid means agree to some 1e-11, and the spectra equal the arbiter's to 1e-14.
    Measured on an MI355X, 3 members, largest by level: 4.4e-6, 2.6e-4, 5.5e-6, 5.2e-5, 4.6e-5, 3.8e-5, 4.7e-5, 3.0e-5."""
    import torch
    members = 3
    model = perturbed(spectral, bc, members)
    model.spectra_configure(("ke_rot_spectrum", "ke_div_spectrum"), 36, 1)
    model.run(36)
    got = {n: model.spectra(n)[:, 0] for n in ("ke_rot_spectrum", "ke_div_spectrum")}
    tables = np.load(golden_dir + "/tables.npz")  # (the reference's tables: nothing of the library under test)
    # the oracle's side of the same comparison, on the state as the device holds it
    rel_oracle = np.zeros((members, 8))
    for i in range(members):
        vor, div = model.get("vor", i)[..., 0], model.get("div", i)[..., 0]  # time level 1
        zero3, zero2 = np.zeros_like(vor), np.zeros_like(vor[:, :, 0])
        want = ref.spectra(vor, div, zero3, zero3, zero2, tables["elm2"])
        for k in range(8):
            us, vs = oracle.vort2vel(vor[:, :, k], div[:, :, k])
            ug, vg = oracle.spec2grid(us, 2), oracle.spec2grid(vs, 2)
            ke = ref.area_mean(0.5 * (ug * ug + vg * vg), tables["wt"])
            rel_oracle[i, k] = abs(float((want["ke_rot_spectrum"][k] + want["ke_div_spectrum"][k]).sum()) / ke - 1.0)
    model.spectral2grid()
    u, v = model.device_view("u_grid").double(), model.device_view("v_grid").double()  # [M][8][48][96]
    wt = torch.as_tensor(tables["wt"], dtype=torch.float64, device=u.device)  # 24 weights of a hemisphere, summing to 1
    w48 = 0.5 * torch.cat([wt, wt.flip(0)])
    ke_grid = ((0.5 * (u * u + v * v)).mean(dim=3) * w48).sum(dim=2)  # [M][8]
    ke_spec = (got["ke_rot_spectrum"] + got["ke_div_spectrum"]).sum(dim=2)
    rel = ((ke_spec / ke_grid) - 1.0).abs().cpu().numpy()
    print("kinetic energy, spectra against the export, largest relative difference by level: " +
          ", ".join("%.2e" % x for x in rel.max(axis=0)))
    print("the oracle's own on the same state:                                              " +
          ", ".join("%.2e" % x for x in rel_oracle.max(axis=0)))
    print("largest |device - oracle| of the two: %.2e" % np.abs(rel - rel_oracle).max())
    assert float(ke_grid.min()) > 0.1
    others = [0, 2, 3, 4, 5, 6, 7]
    assert rel[:, others].max() < 2e-4, rel.max(axis=0).tolist()
    assert np.abs(rel - rel_oracle).max() < 1e-10, (rel.max(axis=0).tolist(), rel_oracle.max(axis=0).tolist())
    assert (rel[:, 1] <= rel_oracle[:, 1] + 1e-10).all(), (rel[:, 1].tolist(), rel_oracle[:, 1].tolist())
    assert_same(model.spectrum(["ke_mean"])["ke_mean"], ke_spec, "ke_mean", "ke_mean")
    dhs = torch.as_tensor(tables["dhs"], dtype=torch.float64, device=u.device)
    assert_same(model.spectrum(["ke_column"])["ke_column"], (ke_spec * dhs).sum(dim=1), "ke_column", "ke_column")
    model.close()

PLANS = {
    "serial": dict(),
    "member_groups_2": dict(options=(("member_groups", 2),)),
    "rounds": dict(options=(("block_members", 1),)),
    "checked": dict(checked=True),
    "one_step_calls": dict(calls=(1,) * STEPS),
    "every_3": dict(every=3),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_in_loop_equals_standalone(spectral, bc, twin, plan):
    """One 12-step call with every = 1 (or 3): each sample of each stored name is bitwise what spectrum() gives the twin that ends
    its call at that step (the derived names, torch sums of those: assert_same) -- in the serial plan, with two member groups, in rounds (block_members = 1 with 4
    members), in a checked call, and in 12 calls of one step.  Steps and dates are the twin's, and so is the state after step 12."""
    p = PLANS[plan]
    series, steps, dates, twin_state = twin
    every = p.get("every", 1)
    model = perturbed(spectral, bc, options=p.get("options", ()))
    model.spectra_configure(NAMES, every, STEPS)
    cfg = model.config()
    if plan == "member_groups_2":
        assert cfg["chunks"] == 2
    if plan == "rounds":
        assert cfg["rounds"] == 4
    for n in p.get("calls", (STEPS,)):
        if p.get("checked"):
            failed, _ = model.run_checked(n)
            assert (failed == -1).all()
        else:
            model.run(n)
    picked = [k for k in range(STEPS) if (k + 1) % every == 0]
    info = model.spectra_info()
    assert info == dict(taken=len(picked), held=len(picked), capacity=STEPS, every=every)
    assert model.spectra_steps().tolist() == [steps[k] for k in picked]
    assert model.spectra_times() == [dates[k] for k in picked]
    for n in NAMES + DERIVED:
        assert_same(model.spectra(n), series[n][:, picked], "%s: %s" % (plan, n), n)
    assert not bool((series["ke_rot_spectrum"][:, 0] == series["ke_rot_spectrum"][:, 1]).all())  # (the steps differ ...)
    assert not bool((series["t_spectrum"][0] == series["t_spectrum"][1]).all())                  # (... and so do the members)
    for n, per_member in twin_state.items():
        for i in range(M):
            assert np.array_equal(model.get(n, i), per_member[i]), (plan, n, i)
    model.close()


def test_the_ring_keeps_the_last_samples(spectral, bc, twin):
    """Capacity 5, twelve samples: the five held ones are the twin's samples 8 to 12 in order, with their steps and dates; reads of
    sample windows and of member sub-ranges give the matching slices; reset empties."""
    import torch
    series, steps, dates, _ = twin
    model = perturbed(spectral, bc)
    model.spectra_configure(NAMES, 1, 5)
    model.run(STEPS)
    assert model.spectra_info() == dict(taken=12, held=5, capacity=5, every=1)
    assert model.spectra_steps().tolist() == steps[7:] == [8, 9, 10, 11, 12]
    assert model.spectra_times() == dates[7:] == [datetime(1982, 1, 1) + timedelta(minutes=40 * k) for k in range(8, 13)]
    rows = np.zeros((3, 6), dtype=np.int32)
    assert model._lib.spd_model_spectra_times(model._m, rows.ctypes.data_as(C.POINTER(C.c_int32)), 3) == 3  # (the oldest three)
    assert rows.tolist() == [[8, 1982, 1, 1, 5, 20], [9, 1982, 1, 1, 6, 0], [10, 1982, 1, 1, 6, 40]]
    for n in NAMES + DERIVED:
        whole = model.spectra(n)
        assert_same(whole, series[n][:, 7:], n, n)
        parts = torch.cat([model.spectra(n, t0=0, nt=2), model.spectra(n, t0=2, nt=3)], dim=1)
        assert_same(parts, whole, n + " in two windows", n)
        assert_same(model.spectra(n, first=1, count=2), whole[1:3], n + " members 1, 2", n)
        assert_same(model.spectra(n, first=2, count=2, t0=3, nt=1), whole[2:4, 3:4], n + " members 2, 3, sample 3", n)
    model.spectra_reset()
    assert model.spectra_info() == dict(taken=0, held=0, capacity=5, every=1)
    assert model.spectra("t_mean").shape == (M, 0, 8) and model.spectra_steps().tolist() == [] and model.spectra_times() == []
    model.run(2)  # a ring that is not full
    assert model.spectra_steps().tolist() == [13, 14] and model.spectra("lnps_mean").shape == (M, 2, 1)
    model.close()


def test_nothing_else_moves(spectral, bc, twin):
    """Every registry variable after 12 steps is bitwise that of a run without spectra -- with the spectra alone, and with statistics
    (every 4) and the tape (every 3) on beside them; the statistics, the tape and the spectra each give bitwise what they give alone."""
    import torch
    stat_names, tape_names = ("u_grid", "precnv"), ("t_grid", "precls")
    runs = {}
    for key, with_stats, with_tape, with_spectra in (("none", 0, 0, 0), ("stats", 1, 0, 0), ("tape", 0, 1, 0), ("spectra", 0, 0, 1),
                                                     ("all", 1, 1, 1)):
        model = perturbed(spectral, bc)
        if with_stats:
            model.stats_configure(stat_names, 4, variance=True)
        if with_tape:
            model.tape_configure(tape_names, 3, 4, dtype="float64")
        if with_spectra:
            model.spectra_configure(NAMES, 1, STEPS)
        model.run(STEPS)
        out = {"state": registry(model)}
        if with_stats:
            assert model.stats_samples == 3
            out["stats"] = {n: (model.stats_mean(n).clone(), model.stats_var(n).clone()) for n in stat_names}
        if with_tape:
            assert model.tape_info["taken"] == 4
            out["tape"] = {n: model.tape(n).clone() for n in tape_names}
        if with_spectra:
            assert model.spectra_info()["taken"] == STEPS
            out["spectra"] = {n: model.spectra(n).clone() for n in NAMES}
        torch.cuda.synchronize()
        runs[key] = out
        model.close()
    for key in ("stats", "tape", "spectra", "all"):
        for n, per_member in runs["none"]["state"].items():
            for a, b in zip(per_member, runs[key]["state"][n]):
                assert np.array_equal(a, b), (key, n)
    for n, per_member in twin[3].items():  # (... and the twin's, stepped in calls of one step)
        for a, b in zip(per_member, runs["all"]["state"][n]):
            assert np.array_equal(a, b), ("twin", n)
    for n in stat_names:
        assert_bitwise(runs["all"]["stats"][n][0], runs["stats"]["stats"][n][0], "mean of " + n)
        assert_bitwise(runs["all"]["stats"][n][1], runs["stats"]["stats"][n][1], "variance of " + n)
    for n in tape_names:
        assert_bitwise(runs["all"]["tape"][n], runs["tape"]["tape"][n], "tape of " + n)
    for n in NAMES:
        assert_bitwise(runs["all"]["spectra"][n], runs["spectra"]["spectra"][n], "spectra of " + n)
        assert_bitwise(runs["all"]["spectra"][n], twin[0][n], "spectra of " + n + " against the twin")


def test_lifecycle_and_the_failure_rule(spectral, bc):
    """Reads before configuring and of unconfigured names fail; a subset of the names records only those; configure, reads and
    reset are refused while a checked call is in flight; a checked call that reports a failed range check makes reads fail, naming
    member and step, until the next reset; spd_model_init empties; off frees; spectrum() needs no configuration."""
    import torch
    from pyspeedy_amd._lib import SpeedyHipError
    model = perturbed(spectral, bc, 2)
    with pytest.raises(SpeedyHipError, match="no spectra configured"):
        model.spectra_info()
    with pytest.raises(SpeedyHipError, match="no spectra configured"):
        model.spectra_reset()
    with pytest.raises(SpeedyHipError, match="unknown name"):
        model.spectra_configure(["t_spectrum", "olr"], 1, 4)
    with pytest.raises(SpeedyHipError, match="every"):
        model.spectra_configure(["t_spectrum"], 0, 4)
    with pytest.raises(SpeedyHipError, match="capacity"):
        model.spectra_configure(["t_spectrum"], 1, 0)
    with pytest.raises(SpeedyHipError, match="unknown name"):
        model.spectrum(["t_grid"])
    with pytest.raises(SpeedyHipError, match="member range out of bounds"):
        model.spectrum(["t_mean"], first=1, count=2)
    assert model.spectrum(["lnps_mean"])["lnps_mean"].shape == (2, 1)  # (no configuration needed)
    model.spectra_configure(["ke_column", "lnps_spectrum", "q_mean"], 3, 4)  # (a derived name records what it needs)
    assert model.spectra_info() == dict(taken=0, held=0, capacity=4, every=3)
    model.run(7)
    assert model.spectra_info()["taken"] == 2 and model.spectra_steps().tolist() == [3, 6]
    assert model.spectra("ke_column").shape == (2, 2) and model.spectra("ke_rot_spectrum").shape == (2, 2, 8, 32)
    assert model.spectra("lnps_spectrum").shape == (2, 2, 32) and model.spectra("q_mean").shape == (2, 2, 8)
    assert model.spectra("q_mean").dtype == torch.float64 and model.spectra("q_mean").is_cuda
    with pytest.raises(SpeedyHipError, match="not among the configured"):
        model.spectra("t_spectrum")
    with pytest.raises(SpeedyHipError, match="not among the configured"):
        model.spectra("u_grid")
    with pytest.raises(SpeedyHipError, match="sample range out of bounds"):
        model.spectra("q_mean", t0=1, nt=2)
    with pytest.raises(SpeedyHipError, match="member range out of bounds"):
        model.spectra("q_mean", first=1, count=2)
    buf = torch.empty(8, dtype=torch.float64, device=model.sp.device)
    assert model._lib.spd_model_spectra_read(model._m, b"lnps_spectrum", 0, 2, 0, 2, buf.data_ptr(), 64, None) == -3  # SPD_E_SIZE
    assert model._lib.spd_model_spectra_compute(model._m, (C.c_char_p * 1)(b"t_spectrum"), 1, 0, 2, buf.data_ptr(), 64, None) == -3
    # the sample at step 6 is still what the state gives once the call has ended there
    model.spectra_reset()
    model.run(2)  # step 9
    assert model.spectra_steps().tolist() == [9]
    assert torch.equal(model.spectra("q_mean")[:, 0], model.spectrum(["q_mean"])["q_mean"])
    # a checked call in flight
    stream = model._stream()
    assert model._lib.spd_model_step_checked_begin(model._m, 3, stream) == 0
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.spectra("q_mean")
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.spectra_configure(["q_mean"], 3, 2)
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.spectra_reset()
    with pytest.raises(SpeedyHipError, match="in flight"):
        model.spectrum(["q_mean"])
    failed = np.zeros(2, dtype=np.int32)
    assert model._lib.spd_model_step_checked_end(model._m, failed.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    assert failed.tolist() == [-1, -1] and model.spectra_steps().tolist() == [9, 12]
    # a member out of range: global-mean temperature of 500 K (diagnostics.f90:57-66), as tests/test_tape_gpu.py
    t = model.get("t", 1)
    t[0, 0, :, :] = 500.0 * np.sqrt(2.0)
    model.set("t", t, member=1)
    failed, _ = model.run_checked(3)
    assert failed.tolist() == [-1, 0]
    with pytest.raises(SpeedyHipError, match="invalid until spd_model_spectra_reset: member 1 failed the range check at step 0"):
        model.spectra("q_mean")
    with pytest.raises(SpeedyHipError, match="member 1 failed the range check at step 0"):
        model.spectra("ke_column")
    assert model.spectra_info()["taken"] == 3  # (the count is still told)
    model.spectra_reset()
    assert model.spectra("q_mean").shape == (2, 0, 8)
    # spd_model_init empties the ring as well
    model.init((1982, 1, 1, 0, 0))
    model.run(6)
    assert model.spectra_info()["taken"] == 2 and model.spectra_steps().tolist() == [3, 6]
    model.init((1982, 1, 1, 0, 0))
    assert model.spectra_info()["taken"] == 0 and model.spectra_info()["capacity"] == 4
    # a ring that does not fit the card (2^31 - 1 samples of 2 x 1073 doubles: 37 TB): refused with the bytes asked for, the spectra
    # are off and the model steps as before
    with pytest.raises(SpeedyHipError, match=r"cannot allocate the series \((\d+) bytes asked for: 2147483647 samples of 17168 bytes\)"):
        model.spectra_configure(NAMES, 1, 2 ** 31 - 1)
    with pytest.raises(SpeedyHipError, match="no spectra configured"):
        model.spectra_info()
    model.run(2)
    model.spectra_configure(["q_mean"], 1, 2)
    model.run(2)
    assert model.spectra_steps().tolist() == [3, 4]
    # off
    model.spectra_configure([], 1, 1)
    with pytest.raises(SpeedyHipError, match="no spectra configured"):
        model.spectra("q_mean")
    model.run(3)
    model.close()
