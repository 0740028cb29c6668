"""GPU tier: pressure-level fields and mean sea-level pressure computed on the device (spd_model_plev_*, EnsembleModel.plev, the
six names in the time statistics, Speedy / SpeedyEns.to_dataframe(pressure_levels=...)).

The arbiter is tests/plev_reference.py, a numpy fp64 restatement of the definition that shares nothing with
the kernel; tests/test_plev_cpu.py pins it.  Bounds: max |difference| <= 1e-12 max |field| per variable against the restatement
(the bound of the physics tier), 1e-12 of a field's range for the statistics (the bound of tests/test_stats_gpu.py)."""
import os
import tempfile
from datetime import datetime

import numpy as np
import pytest

from plev_reference import SIGL, plev_reference

pytestmark = pytest.mark.gpu

NAMES = ("u_plev", "v_plev", "t_plev", "q_plev", "z_plev", "mslp")
GRID = (("u", "u_grid"), ("v", "v_grid"), ("t", "t_grid"), ("q", "q_grid"), ("z", "phi_grid"))
# hPa: the ten levels of the issue (925 ... 10 and 1050), in the strictly decreasing order the interface asks for
LEVELS = [1050.0, 925.0, 850.0, 700.0, 500.0, 300.0, 200.0, 100.0, 30.0, 10.0]
EVERY = 9


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


def turned(x):  # (lon, lat[, lev]) -> ([lev,] lat, lon)
    return np.ascontiguousarray(x.transpose(*range(x.ndim - 1, -1, -1)))


def perturbed(spectral, bc, M, fp32=False, options=()):
    """the members of tests/test_stats_gpu.py: t_grid += N(0, 0.01 K), seed = member id"""
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
    return model


def grid_inputs(model):
    """the model's own fp64 grid arrays and phis0, as the restatement takes them ([member][lev][lat][lon])"""
    fields = {n: model.device_view(g).cpu().numpy() for n, g in GRID}
    return fields, model.device_view("ps_grid").cpu().numpy(), model.device_view("phis0").cpu().numpy()


def compare(got, ref, what):
    worst = {}
    for name in NAMES:
        g = got[name].cpu().numpy()
        assert g.shape == ref[name].shape, (name, g.shape, ref[name].shape)
        worst[name] = float(np.abs(g - ref[name]).max()), float(np.abs(ref[name]).max())
    print(what, {n: "%.2e of %.3g" % w for n, w in worst.items()})
    for name, (err, size) in worst.items():
        assert err <= 1e-12 * size, (what, name, err, size)
    return worst


def test_against_the_reference_data(spectral, bc, golden_dir):
    """The reference's own exported one-day fields written into the grid arrays (bit for bit its numbers), its phis0, and all six
    outputs at ten levels against the restatement on the same arrays.  No point is left out: 14.7 / 8.8 / 3.0 % of the columns
    are under the ground at 925 / 850 / 700 hPa and 23.5 / 11.7 / 4.2 % below level 7, 10 hPa is above the top level everywhere."""
    import torch
    from pyspeedy_amd.model import EnsembleModel
    e, r = np.load(golden_dir + "/export.npz"), np.load(golden_dir + "/run.npz")
    model = EnsembleModel(spectral, 1)
    model.set_bc(bc, start_date=(1982, 1, 1, 0, 0))
    model.set("phis0", r["d1_phis0"])
    fields = {}
    for n, g in GRID + (("ps", "ps_grid"),):
        fields[n] = turned(e["d1_" + g])[None]
        view = model.device_view(g)
        view.copy_(torch.from_numpy(fields[n]))
        assert np.array_equal(view.cpu().numpy(), fields[n])
    ps = fields.pop("ps")
    phis0 = turned(r["d1_phis0"])[None]
    s925 = np.log(92500.0 / ps)
    assert (ps < 92500.0).mean() > 0.10 and (s925 > SIGL[7]).mean() > 0.20 and (np.log(1000.0 / ps) < SIGL[0]).all()
    model.plev_configure(LEVELS)
    assert model.plev_levels == tuple(LEVELS)
    got = model.plev(refresh=False)
    compare(got, plev_reference(fields, ps, phis0, [p * 100.0 for p in LEVELS]), "reference day 1")
    model.close()


@pytest.mark.parametrize("M", [1, 3, 64])
def test_developed_state(spectral, bc, M):
    """Perturbed members after 72 steps, against the restatement on the model's own grid arrays; descending and ascending level
    lists give the same planes bitwise; a member sub-range equals the slice of the full call bitwise."""
    import torch
    model = perturbed(spectral, bc, M)
    model.run(72)
    down = sorted(LEVELS, reverse=True)
    model.plev_configure(down)
    got = model.plev()
    torch.cuda.synchronize()
    fields, ps, phis0 = grid_inputs(model)
    compare(got, plev_reference(fields, ps, phis0, [p * 100.0 for p in down]), "%d members, 72 steps" % M)
    model.plev_configure(down[::-1])
    assert model.plev_levels == tuple(down[::-1])
    up = model.plev()
    for name in NAMES:
        assert torch.equal(up[name], got[name].flip(1) if name != "mslp" else got[name]), name
    first, count = (0, 1) if M == 1 else (1, 2) if M == 3 else (37, 20)
    some = model.plev(first=first, count=count, refresh=False)
    few = model.plev(names=["z_plev", "mslp"], first=first, count=count)
    assert sorted(few) == ["mslp", "z_plev"]
    for name in NAMES:
        assert some[name].shape[0] == count
        assert torch.equal(some[name], up[name][first:first + count]), name
    for name in few:
        assert torch.equal(few[name], up[name][first:first + count]), name
    model.close()


STATE = ("vor", "div", "t", "tr", "ps")
GRIDS = ("u_grid", "v_grid", "t_grid", "q_grid", "phi_grid", "ps_grid", "precnv", "precls")


def test_nothing_else_moves(spectral, bc):
    """plev() leaves the spectral state and all eight grid arrays bitwise what spectral2grid() alone leaves; a model that has
    levels configured but is only stepped ends 72 steps bitwise equal to one that never heard of them."""
    M = 3
    results = []
    for with_levels in (False, True):
        model = perturbed(spectral, bc, M)
        if with_levels:
            model.plev_configure([850.0, 500.0])
        model.run(72)
        stepped = {n: [model.get(n, i) for i in range(M)] for n in model.variables() if n not in ("lon", "lat", "lev")}
        model.spectral2grid()
        if with_levels:
            model.plev()
        after = {n: [model.get(n, i) for i in range(M)] for n in STATE + GRIDS}
        results.append((stepped, after))
        model.close()
    for part in (0, 1):
        for n, per_member in results[0][part].items():
            for a, b in zip(per_member, results[1][part][n]):
                assert np.array_equal(a, b), (part, n)


# ---- statistics ------------------------------------------------------------------------------------------------------------
STAT_LEVELS = [500.0, 850.0]
PLANS = {
    "one_group_8": dict(M=8, calls=(36, 36)),
    "two_groups_64": dict(M=64, calls=(36, 36)),
    "rounds_32": dict(M=32, calls=(36, 36), options=(("block_members", 4),), checked=True),
    "fp32_storage_8": dict(M=8, calls=(36, 36), fp32=True),
    "one_step_calls_8": dict(M=8, calls=(1,) * 72),
    "mixed_8": dict(M=8, calls=(36, 36), names=("z_plev", "t_grid", "precnv")),
}
STAT_NAMES = ("z_plev", "t_plev", "u_plev", "mslp")


def step(model, n, checked):
    if checked:
        failed, _ = model.run_checked(n)
        assert (failed == -1).all()
    else:
        model.run(n)


def twin_statistics(spectral, bc, M, names, samples, fp32, options):
    """the loop a user writes by hand: a call ends at every sample, plev() (or a read of the registry variable), shifted sums on
    the host"""
    import torch
    model = perturbed(spectral, bc, M, fp32, options)
    model.plev_configure(STAT_LEVELS)
    views = {n: model.device_view(n) for n in names if n not in NAMES}
    shift, s1, s2 = {}, {}, {}
    for k in range(samples):
        model.run(EVERY)
        fields = model.plev([n for n in names if n in NAMES])
        torch.cuda.synchronize()
        for n in names:
            x = (fields[n] if n in NAMES else views[n].double()).cpu().numpy()
            if k == 0:
                shift[n], s1[n], s2[n] = x, np.zeros_like(x), np.zeros_like(x)
            d = x - shift[n]
            s1[n] += d
            s2[n] += d * d
    mean = {n: shift[n] + s1[n] / samples for n in names}
    var = {n: (s2[n] - s1[n] * s1[n] / samples) / (samples - 1) for n in names}
    state = {n: [model.get(n, i) for i in range(M)] for n in STATE}
    model.close()
    return mean, var, state


def scaled(got, ref):
    return float(np.abs(got - ref).max() / max(float(ref.max() - ref.min()), 1e-300))


@pytest.mark.parametrize("plan", list(PLANS))
def test_statistics_equal_the_hand_rolled_loop(spectral, bc, plan):
    """Mean and variance of z_plev, t_plev, u_plev (500 and 850 hPa) and mslp sampled every 9 steps over 72, against the twin, to
    1e-12 of each field's range; the final spectral state is bitwise the twin's, which never configured statistics."""
    p = PLANS[plan]
    M, options, fp32, checked = p["M"], p.get("options", ()), p.get("fp32", False), p.get("checked", False)
    names = p.get("names", STAT_NAMES)
    samples = sum(p["calls"]) // EVERY
    mean, var, twin_state = twin_statistics(spectral, bc, M, names, samples, fp32, options)
    model = perturbed(spectral, bc, M, fp32, options)
    model.plev_configure(STAT_LEVELS)
    for n in names:
        if n not in NAMES:
            model.device_view(n)  # (as the twin: taking a view drops derived state)
    model.stats_configure(names, EVERY, variance=True)
    cfg = model.config()
    if plan == "two_groups_64":
        assert cfg["chunks"] == 2
    if plan == "rounds_32":
        assert cfg["rounds"] > 1
    if plan == "fp32_storage_8":
        assert cfg["physics_storage32"]
    for n in p["calls"]:
        step(model, n, checked)
    assert model.stats_samples == samples
    worst = {}
    for n in names:
        got_mean, got_var = model.stats_mean(n).cpu().numpy(), model.stats_var(n).cpu().numpy()
        expect = (M, 48, 96) if n in ("mslp", "precnv") else (M, 8, 48, 96) if n == "t_grid" else (M, len(STAT_LEVELS), 48, 96)
        assert got_mean.shape == got_var.shape == expect, (n, got_mean.shape)
        worst[n] = (scaled(got_mean, mean[n]), scaled(got_var, var[n]))
    print(plan, {n: "%.1e / %.1e" % w for n, w in worst.items()})
    for n, (em, ev) in worst.items():
        assert em <= 1e-12 and ev <= 1e-12, (n, em, ev)
    for n, per_member in twin_state.items():
        for i in range(M):
            assert np.array_equal(model.get(n, i), per_member[i]), (n, i)
    model.close()


def test_ensemble_reduction(spectral, bc):
    """stats_ensemble of z_plev and mslp against torch over the members (1e-13 of the values reduced, as tests/test_stats_gpu.py)."""
    import torch
    model = perturbed(spectral, bc, 8)
    model.plev_configure(STAT_LEVELS)
    model.stats_configure(["z_plev", "mslp"], EVERY, variance=False)
    model.run(36)
    for n in ("z_plev", "mslp"):
        per_member = model.stats_mean(n)
        mean, std = model.stats_ensemble(n)
        ref_mean, ref_std = torch.mean(per_member, dim=0), torch.std(per_member, dim=0, unbiased=True)
        assert mean.shape == ref_mean.shape == per_member.shape[1:]
        scale = float(per_member.abs().max())
        assert float((mean - ref_mean).abs().max()) <= 1e-13 * scale, n
        assert float((std - ref_std).abs().max()) <= 1e-13 * scale, n
        assert float(ref_std.max()) > 0.0, n
    model.close()


def test_arguments(spectral, bc):
    """Every refusal comes with SPD_E_ARG and a message, and the model steps and exports as before afterwards."""
    import torch
    from pyspeedy_amd import _lib
    from pyspeedy_amd._lib import SpeedyHipError
    model, twin = perturbed(spectral, bc, 2), perturbed(spectral, bc, 2)
    L = model._lib

    def refused(call, match):
        with pytest.raises(SpeedyHipError, match=match) as info:
            call()
        assert "(%d)" % _lib.SPD_E_ARG in str(info.value), str(info.value)

    refused(lambda: model.stats_configure(["z_plev"], EVERY), "needs target levels")
    refused(lambda: model.plev(), "no target levels")
    refused(lambda: model.plev_configure([850.0, 500.0, 700.0]), "strictly")
    refused(lambda: model.plev_configure([850.0, 850.0]), "strictly")
    refused(lambda: model.plev_configure([500.0, 0.0]), "positive")
    refused(lambda: model.plev_configure([500.0, -10.0]), "positive")
    refused(lambda: model.plev_configure([1000.0 - 10.0 * j for j in range(33)]), "at most 32")
    assert model.plev_levels == ()
    model.plev_configure([1000.0 - 10.0 * j for j in range(32)])
    assert len(model.plev_levels) == 32 and model.plev()["z_plev"].shape == (2, 32, 48, 96)
    model.plev_configure([850.0, 500.0])
    refused(lambda: model.plev(["z_plev", "olr"]), "unknown variable")
    refused(lambda: model.plev(["t_grid"]), "unknown variable")
    refused(lambda: model.plev(first=1, count=2), "out of bounds")
    buf = torch.empty(8, dtype=torch.float64, device=model.sp.device)
    assert L.spd_model_plev_read(model._m, b"q_plev", 0, 2, buf.data_ptr(), 64, None) == _lib.SPD_E_ARG  # (never computed)
    model.plev(["q_plev"])
    assert L.spd_model_plev_read(model._m, b"q_plev", 0, 2, buf.data_ptr(), 64, None) == _lib.SPD_E_SIZE
    model.stats_configure(["z_plev", "ps_grid"], EVERY)
    refused(lambda: model.plev_configure([700.0]), "statistics")
    refused(lambda: model.plev_configure([]), "statistics")
    assert model.plev_levels == (850.0, 500.0)
    model.stats_configure([], EVERY)
    model.plev_configure([700.0])
    assert model.plev()["z_plev"].shape == (2, 1, 48, 96)
    model.plev_configure([])
    assert model.plev_levels == ()
    # ... and the model steps and exports as one that was never asked any of this
    for m in (model, twin):
        m.run(9)
        m.spectral2grid()
    for n in STATE + GRIDS:
        for i in range(2):
            assert np.array_equal(model.get(n, i), twin.get(n, i)), n
    model.close()
    twin.close()


# ---- facade ----------------------------------------------------------------------------------------------------------------
def check_frame(frame, plain, owners, ens, levels):
    """owners: the Speedy objects along `ens` (one object and ens = False: a single run, no such dimension)"""
    from pyspeedy_amd import speedy_driver as drv
    lead = ("time", "ens") if ens else ("time",)
    assert frame["plev"].dims == ("plev",) and frame["plev"].values.tolist() == levels
    assert frame["plev"].attrs["units"] == "hPa" and frame["plev"].attrs["positive"] == "down"
    for name in NAMES:
        v = frame[name]
        assert v.values.dtype == np.float32, name
        assert v.dims == lead + (("plev",) if name != "mslp" else ()) + ("lat", "lon"), (name, v.dims)
        assert v.shape == (1,) + ((len(owners),) if ens else ()) + ((len(levels),) if name != "mslp" else ()) + (48, 96)
    for name, v in plain.data_vars.items():
        assert np.array_equal(frame[name].values, v.values), name
        assert frame[name].dims == v.dims
    assert frame["lev"].values.tolist() == plain["lev"].values.tolist()
    for pos, owner in enumerate(owners):
        model, index = drv.device_model(owner._state_cnt)
        assert model.plev_levels == tuple(levels)
        ref = model.plev(first=index, count=1)
        for name in NAMES:
            got = frame[name].values[0, pos] if ens else frame[name].values[0]
            assert np.array_equal(got, ref[name][0].float().cpu().numpy()), name


def roundtrip(frame):
    from pyspeedy_amd.dataset import open_dataset, write_netcdf
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "plev.nc")
        write_netcdf(frame, path)
        back = open_dataset(path)
    assert back["plev"].values.dtype == np.float32 and np.array_equal(back["plev"].values, frame["plev"].values)
    assert back["plev"].attrs["units"] == "hPa" and back["plev"].attrs["positive"] == "down"
    for name, v in frame.data_vars.items():
        assert back[name].dims == v.dims, name
        assert np.array_equal(back[name].values, v.values), name


def test_facade_single(bc):
    """Speedy after a day: to_dataframe(pressure_levels=[850, 500])."""
    from pyspeedy_amd.speedy import Speedy
    model = Speedy(start_date=datetime(1982, 1, 1), end_date=datetime(1982, 1, 2))
    model.set_bc()
    model.run()
    plain = model.to_dataframe()
    frame = model.to_dataframe(pressure_levels=[850, 500])
    check_frame(frame, plain, [model], model.is_ensemble_member, [850.0, 500.0])
    z500 = frame["z_plev"].values[0, 1]
    assert 4500.0 < z500.min() and z500.max() < 6200.0
    roundtrip(frame)
    with pytest.raises(ValueError, match="packed"):
        model.to_dataframe(packed=True, pressure_levels=[850, 500])
    again = model.to_dataframe()
    assert "plev" not in again and "z_plev" not in again
    for name, v in plain.data_vars.items():
        assert np.array_equal(again[name].values, v.values), name


def test_facade_ensemble(bc):
    """SpeedyEns(3) after a day."""
    from pyspeedy_amd.speedy import SpeedyEns
    ens = SpeedyEns(3, start_date=datetime(1982, 1, 1), end_date=datetime(1982, 1, 2))
    for member in ens:
        member.set_bc()
    t = ens.members[1]["t_grid"]
    ens.members[1]["t_grid"] = t + np.random.default_rng(1).normal(0.0, 0.01, t.shape)
    ens.members[1].grid2spectral()
    ens.run()
    plain = ens.to_dataframe()
    frame = ens.to_dataframe(pressure_levels=[850, 500])
    check_frame(frame, plain, list(ens), True, [850.0, 500.0])
    assert not np.array_equal(frame["z_plev"].values[0, 0], frame["z_plev"].values[0, 1])
    assert np.array_equal(frame["z_plev"].values[0, 0], frame["z_plev"].values[0, 2])
    roundtrip(frame)
    with pytest.raises(ValueError, match="packed"):
        ens.to_dataframe(packed=True, pressure_levels=[850, 500])
