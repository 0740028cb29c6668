"""GPU tier: derived fields computed on the device (spd_model_derive_*, EnsembleModel.derived, the fourteen names in the tape, the
statistics, the projection tape and the window tape).

The arbiter is tests/derive_reference.py, a numpy fp64 restatement of the definitions that shares nothing
with the kernel; tests/test_derive_cpu.py pins it.  Its u, v, T, q, ps, vor, div are read from the device, its grad ln ps comes
from the CPU oracle's gradient and inverse transform of the model's ln ps.  Bounds: max |difference| <= 1e-12 max |field| per
name (the bound of DESIGN section 4b); for omega, whose terms cancel and whose grad ln ps comes from another implementation of
the transform, 1e-12 of the maximum over the field of ps sum_k dhs[k] (|u px| + |v py| + |D|).  A sampled field against
derived() at that step of a twin: BITWISE.  Statistics: 1e-13 of the field's range."""
import numpy as np
import pytest

import derive_reference as ref
import projtape_reference as proj

pytestmark = pytest.mark.gpu

NAMES = ref.NAMES
# hPa: under the ground and below level 7 in places (1050, 925), inside (500, 200), above the top full level (30 in places, 10)
LEVELS = [1050.0, 925.0, 500.0, 200.0, 30.0, 10.0]
SHAPES = {"1_member": (1, ()), "3_members": (3, ()), "8_members_2_groups_2_rounds": (8, (("member_groups", 2), ("block_members", 2)))}
GRID = (("u", "u_grid"), ("v", "v_grid"), ("t", "t_grid"), ("q", "q_grid"))
SPINUP, EVERY, STEPS = 72, 4, 12


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


def developed(spectral, bc, shape, levels=LEVELS):
    """the members of tests/test_tape_gpu.py (t_grid += N(0, 0.01 K), seed = member id) after 72 steps, target levels configured"""
    from test_tape_gpu import perturbed
    M, options = SHAPES[shape]
    model, views = perturbed(spectral, bc, M, options=options, levels=levels)
    model.run(SPINUP)
    return model, views


def assert_bitwise(got, want, what):
    import torch
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = got != want
        raise AssertionError("%s: %d of %d values differ, max |diff| %.3e" % (
            what, int(bad.sum()), bad.numel(), float((got.double() - want.double()).abs().max())))


def oracle_gradient(oracle, model, M):
    """grad ln ps of every member from the CPU oracle: gradient() of the spectral ln ps read through get(), then the inverse
    transform with kcos = 2 -> px, py as [M][48][96]"""
    px, py = [], []
    for i in range(M):
        ps = model.get("ps", i)
        ps = ps[..., 0] if ps.ndim == 3 else ps  # (time level 1, the level the export transforms read)
        dx, dy = oracle.gradient(np.asfortranarray(ps))
        px.append(oracle.spec2grid(dx, kcos=2).T)
        py.append(oracle.spec2grid(dy, kcos=2).T)
    return np.stack(px), np.stack(py)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_name_against_the_arbiter(spectral, bc, oracle, shape):
    """derived() of all fourteen names on a developed state against the numpy restatement; a member sub-range and a subset of the
    names equal the slices of the full call bitwise; the columns cover under the ground, below level 7, inside, above level 0."""
    import torch
    model, views = developed(spectral, bc, shape)
    M = SHAPES[shape][0]
    got = model.derived()
    torch.cuda.synchronize()
    assert tuple(got) == NAMES
    fields = {n: views[g].cpu().numpy() for n, g in GRID}
    fields["vor"], fields["div"] = got["vor_grid"].cpu().numpy(), got["div_grid"].cpu().numpy()
    ps = views["ps_grid"].cpu().numpy()
    px, py = oracle_gradient(oracle, model, M)
    s = np.log(np.asarray(LEVELS)[:, None, None, None] * 100.0 / ps[None])
    assert (ps < 105000.0).any() and (s[1] > ref.SIGL[7]).any() and (s[1] <= ref.SIGL[7]).any()
    assert ((s[3] >= ref.SIGL[0]) & (s[3] <= ref.SIGL[7])).all() and (s[2] <= ref.SIGL[7]).any() and (s[5] < ref.SIGL[0]).all()
    want = ref.derive_reference(fields, ps, px, py, [p * 100.0 for p in LEVELS])
    scale = float(ref.omega_scale(fields["u"], fields["v"], fields["div"], ps, px, py).max())
    worst = {}
    for name in NAMES:
        g = got[name].cpu().numpy()
        assert g.shape == want[name].shape, (name, g.shape, want[name].shape)
        size = scale if name.startswith("omega") else float(np.abs(want[name]).max())
        worst[name] = float(np.abs(g - want[name]).max()), size
    print(shape, {n: "%.2e of %.3g" % w for n, w in worst.items()})
    for name, (err, size) in worst.items():
        assert size > 0.0 and err <= 1e-12 * size, (shape, name, err, size)
    first, count = (0, 1) if M == 1 else (1, 2) if M == 3 else (3, 4)
    some = model.derived(first=first, count=count, refresh=False)
    few = model.derived(names=["omega_plev", "tcwv", "vor_grid"], first=first, count=count)
    assert sorted(few) == ["omega_plev", "tcwv", "vor_grid"]
    for name in NAMES:
        assert_bitwise(some[name], got[name][first:first + count], name)
    for name in few:
        assert_bitwise(few[name], got[name][first:first + count], name)
    model.close()


def test_a_resting_state(spectral, bc):
    """vor = div = 0 and a surface pressure with a gradient: omega is 0.0 in every bit on sigma and pressure levels, the
    integrals of the wind and the vorticity are 0.0, and what does not depend on the wind is not."""
    import torch
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, 1)
    model.set_bc(bc, start_date=(1982, 1, 1, 0, 0))
    for name in ("vor", "div"):
        dtype, shape = model.shape(name)
        model.set(name, np.zeros(shape, dtype=dtype))
    model.plev_configure(LEVELS)
    got = model.derived()
    torch.cuda.synchronize()
    ps = model.device_view("ps_grid")
    assert float(ps.max() - ps.min()) > 1.0e4
    for name in ("omega_grid", "omega_plev"):
        assert got[name].numel() > 0 and int(got[name].view(torch.int64).abs().max()) == 0, name
    for name in ("ke_col", "ivt_u", "ivt_v", "vor_grid", "vor_plev", "div_grid"):
        assert bool((got[name] == 0.0).all()), name
    assert float(got["tcwv"].max()) > 0.0 and float(got["theta_grid"].min()) > 200.0
    model.close()


class World:
    """One shape: model `a` records everything inside one run(12); twin `b` is stepped by run(4) calls with derived() after each;
    model `c` takes twelve run(1) calls with the same tape."""

    def __init__(self, spectral, bc, shape):
        import torch
        self.M = SHAPES[shape][0]
        weights = np.zeros((1, 48, 96))
        weights[0, 20:30, 10:40] = 1.0 / 300.0  # a box mean
        self.weights = weights
        a, _ = developed(spectral, bc, shape)
        a.tape_configure(NAMES, EVERY, STEPS // EVERY, dtype="float64")
        a.stats_configure(["omega_plev", "tcwv"], EVERY, variance=False)
        a.projtape_configure(weights, [("tcwv", 0, 0)], EVERY, STEPS // EVERY)
        a.run(STEPS)
        self.tape = {n: a.tape(n).clone() for n in NAMES}
        self.tape_steps = a.tape_steps()
        self.mean = {n: a.stats_mean(n).clone() for n in ("omega_plev", "tcwv")}
        self.samples = a.stats_samples
        self.series = a.projtape().clone()
        a.close()
        b, _ = developed(spectral, bc, shape)
        self.twin = {n: [] for n in NAMES}
        for _ in range(STEPS // EVERY):
            b.run(EVERY)
            for n, x in b.derived().items():
                self.twin[n].append(x.clone())
        self.twin = {n: torch.stack(v, dim=1) for n, v in self.twin.items()}
        b.close()
        c, _ = developed(spectral, bc, shape)
        c.tape_configure(NAMES, EVERY, STEPS // EVERY, dtype="float64")
        for _ in range(STEPS):
            c.run(1)
        self.tape_single = {n: c.tape(n).clone() for n in NAMES}
        c.close()
        torch.cuda.synchronize()


@pytest.fixture(scope="module", params=list(SHAPES))
def world(request, spectral, bc):
    return World(spectral, bc, request.param)


def test_tape_of_all_fourteen_names(world):
    """an fp64 tape sampled every 4 steps inside one run(12): every slot is derived() at that step of the twin, bit for bit, and
    twelve run(1) calls leave the same tape"""
    assert list(world.tape_steps) == [SPINUP + EVERY * (k + 1) for k in range(STEPS // EVERY)]
    for name in NAMES:
        assert world.tape[name].shape[:2] == (world.M, STEPS // EVERY)
        assert_bitwise(world.tape[name], world.twin[name], name)
        assert_bitwise(world.tape_single[name], world.tape[name], name + ", one-step calls")
    assert float(world.tape["omega_grid"].abs().max()) > 1e-3 and float(world.tape["tcwv"].min()) > 0.0


def test_statistics(world):
    """the mean of omega_plev and tcwv over the 3 samples against the host loop over derived(): within 1e-13 of the field's range"""
    assert world.samples == STEPS // EVERY
    for name in ("omega_plev", "tcwv"):
        want = world.twin[name].mean(dim=1)
        spread = float(want.max() - want.min())
        err = float((world.mean[name] - want).abs().max())
        print(name, "%.2e of %.3g" % (err, spread))
        assert spread > 0.0 and err <= 1e-13 * spread, (name, err, spread)


def test_projection_tape(world):
    """one entry, tcwv under a box pattern: the sum of DESIGN section 4j of the fp64 tape's planes, bitwise"""
    import torch
    want = proj.project(world.weights[0], world.tape["tcwv"].cpu().numpy())
    assert world.series.shape == (world.M, STEPS // EVERY, 1)
    assert_bitwise(world.series[..., 0].cpu(), torch.from_numpy(want), "tcwv box mean")
    assert 1.0 < float(want.min()) and float(want.max()) < 80.0  # (kg/m^2)


def test_window_tape(spectral, bc):
    """the maximum of omega_grid over a window of 4 samples equals the reduction of an fp64 tape of the same samples"""
    model, _ = developed(spectral, bc, "3_members")
    model.tape_configure(["omega_grid"], 3, 4, dtype="float64")
    model.wintape_configure([("omega_grid", "max")], 12, 1, sample_every=3, dtype="float64")
    model.run(12)
    samples, steps = model.wintape_counts()
    assert list(samples) == [4] and list(steps) == [12]
    tape = model.tape("omega_grid")
    assert tape.shape[:2] == (3, 4)
    assert_bitwise(model.wintape("omega_grid", "max")[:, 0], tape.max(dim=1).values, "max of omega_grid")
    model.close()


def test_a_configuration_without_the_new_names(spectral, bc):
    """a tape of t_grid, z_plev and mslp over 12 steps is what spectral2grid() and plev() give a twin stepped by run(4) calls,
    bitwise, and the call leaves option quiet_rim_members as a plain run does"""
    import torch
    model, _ = developed(spectral, bc, "3_members")
    model.tape_configure(["t_grid", "z_plev", "mslp"], EVERY, STEPS // EVERY, dtype="float64")
    model.run(STEPS)
    tape = {n: model.tape(n).clone() for n in ("t_grid", "z_plev", "mslp")}
    rim = model.get_option("quiet_rim_members")
    model.close()
    plain, _ = developed(spectral, bc, "3_members")
    plain.run(STEPS)
    assert plain.get_option("quiet_rim_members") == rim
    plain.close()
    twin, views = developed(spectral, bc, "3_members")
    want = {n: [] for n in tape}
    for _ in range(STEPS // EVERY):
        twin.run(EVERY)
        twin.spectral2grid()
        want["t_grid"].append(views["t_grid"].double().clone())
        for n, x in twin.plev(["z_plev", "mslp"]).items():
            want[n].append(x.clone())
    for n in tape:
        assert_bitwise(tape[n], torch.stack(want[n], dim=1), n)
    twin.close()


def test_levels_are_needed_and_held(spectral, bc):
    """a pressure-level name is refused without target levels, by derived() and by a recorder; plev_configure is refused while a
    recorder holds one; the other names need no levels"""
    from pyspeedy_amd._lib import SpeedyHipError
    model, _ = developed(spectral, bc, "1_member", levels=())
    with pytest.raises(SpeedyHipError, match="needs target levels"):
        model.derived(["tcwv", "theta_plev"])
    with pytest.raises(SpeedyHipError, match="needs target levels"):
        model.tape_configure(["vor_plev"], EVERY, 2)
    with pytest.raises(SpeedyHipError, match="unknown variable"):
        model.derived(["t_grid"])
    got = model.derived()
    assert tuple(got) == NAMES[:9]
    model.plev_configure(LEVELS)
    model.tape_configure(["vor_plev"], EVERY, 2)
    with pytest.raises(SpeedyHipError, match="the tape holds a pressure-level variable"):
        model.plev_configure([500.0])
    model.tape_configure([], EVERY, 2)
    model.plev_configure([500.0])
    assert model.derived(["rh_plev"])["rh_plev"].shape == (1, 1, 48, 96)
    model.close()
