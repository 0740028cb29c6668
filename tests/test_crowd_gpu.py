"""GPU tier: every in-loop consumer in ONE model against the model that carries it alone (tests/crowd_cases.py holds the
configuration and the schedule, tests/test_crowd_cpu.py the conditions on them).

Each feature's own test file pins it to its numpy arbiter; what nothing held until now is the code they share when all of them are
due in one call: the cuts of `step_impl` at three periods at once and the order of the events there, the per-segment bookkeeping of
`step_segment` (partition, quiet rim, schedule of the compact longwave record, seven cursors and two open windows), the union in
`decide_step` that decides whether a step stores its diagnostics-only outputs, and, with fp32 physics storage, precnv / precls read
as float by the verification and the quantile tape.  The property needs no tolerance: a consumer's ring in the crowd holds the bits
it holds alone, and the state holds the bits it has under the state-changing features only.

Per (plan, driver) -- drivers: A nudging + in-loop orthonormalised breeding, B nudging + in-loop assimilation -- these models start
from one recipe (perturbed, plev_configure, run to step 30) and are stepped through the same calls of 5, 1, 7, 12, 3 and 20 steps:
`still` (nothing), `bare` (the drivers), `crowd` (drivers + nine recorders + verification + quantile tape), `crowd_checked` (the same
through run_checked) and eleven `solo` models (drivers + one consumer).  The derived-field and pressure-level stages have no ring of
their own: they are looked at through the fp64 tape, whose solo models name only derived / only pressure-level variables while the
crowd's stages compute the union that all of its recorders ask for.

  1  the state of the crowd is the state of `bare`, in every registry variable; the checked calls report no failure
  2  every array, stamp and counter a consumer hands out in the crowd is the one it hands out alone; checked equals unchecked
  3  the drivers' own rings in the crowd are those of `bare`
  4  every ring's stamps are what the Python schedule predicts; the small rings hold the last `capacity` of them
  5  anchors on the crowd's own fp64 tape (sampled every step), so that crowd and solo cannot be wrong together: the projection
     rows, the verification's phase 0, the quantile planes; with driver B the verification's phase 1 against the arbiter on the
     state a host loop's analysis left
  6  without joined consumers and events: nine recorders + nudging in one call of 40 steps (one segment, second group offset)
  7  *_off() of one consumer after the other, 7 steps behind each: the others continue as their solo models do, windows that
     were open across the switch close with the same bits and counts, and the state stays that of `bare`

The window recorders expose no view of their open window; its start and sample count are held through the windows that close in 7
(the accumulation tape's window open since step 76 closes at 80 with 4 steps, the window tape's of 78 at 84 with 3 samples)."""
import time

import numpy as np
import pytest

import crowd_cases as cc
import projtape_reference as proj
import qtape_reference as qref
import verif_reference as vref
from test_breed_gpu import SPEC, bc, bits, differing, perturb, registry  # noqa: F401

pytestmark = pytest.mark.gpu

COMPARED = [0]  # arrays compared bitwise by `mismatches`, for the record (profiles/crowd_parity.txt)
WALL = {}


@pytest.fixture(scope="module")
def maps():
    w = cc.weight_maps()
    assert (w[0] > 0).all() and 0 < np.count_nonzero(w[1]) < 4608 and w[2].all() and np.count_nonzero(w[3]) == 4
    return w


def host(t):
    return t.cpu().numpy()


# ---- the consumers: how each is switched on, read and switched off -------------------------------------------------------------------
def tape_on(names):
    return lambda m, plan, maps: m.tape_configure(names, cc.EVERY["tape"], cc.CAPACITY["tape"], dtype="float64")


CONFIGURE = {
    "stats": lambda m, plan, maps: m.stats_configure(cc.STATS, cc.EVERY["stats"], variance=True),
    "tape": tape_on(cc.TAPED),
    "derive": tape_on(cc.DERIVE_TAPED),
    "plev": tape_on(cc.PLEV_TAPED),
    "spectra": lambda m, plan, maps: m.spectra_configure(cc.SPECTRA, cc.EVERY["spectra"], cc.CAPACITY["spectra"]),
    "enstape": lambda m, plan, maps: m.enstape_configure(cc.ENSTAPE, cc.EVERY["enstape"], cc.CAPACITY["enstape"]),
    "acctape": lambda m, plan, maps: m.acctape_configure(cc.ACCTAPE, cc.EVERY["acctape"], cc.CAPACITY["acctape"], dtype="float64"),
    "wintape": lambda m, plan, maps: m.wintape_configure(cc.WINTAPE, cc.EVERY["wintape"], cc.CAPACITY["wintape"],
                                                         sample_every=cc.WIN_SAMPLE_EVERY, dtype="float64"),
    "projtape": lambda m, plan, maps: m.projtape_configure(maps, cc.PROJTAPE, cc.EVERY["projtape"], cc.CAPACITY["projtape"]),
    "verif": lambda m, plan, maps: m.verif_configure(maps, cc.VERIF, plan["verif"][0], plan["verif"][1], cc.VERIF_EVERY,
                                                     capacity=cc.CAPACITY["verif"]),
    "qtape": lambda m, plan, maps: m.qtape_configure(cc.QTAPE, plan["qtape"], cc.QTAPE_EVERY, capacity=cc.CAPACITY["qtape"]),
}
OFF = {
    "stats": lambda m, maps: m.stats_configure([], cc.EVERY["stats"]),
    "tape": lambda m, maps: m.tape_configure([], cc.EVERY["tape"], 1),
    "spectra": lambda m, maps: m.spectra_configure([], cc.EVERY["spectra"], 1),
    "enstape": lambda m, maps: m.enstape_configure([], cc.EVERY["enstape"], 1),
    "acctape": lambda m, maps: m.acctape_configure([], cc.EVERY["acctape"], 1),
    "wintape": lambda m, maps: m.wintape_configure([], cc.EVERY["wintape"], 1),
    "projtape": lambda m, maps: m.projtape_configure(maps, [], cc.EVERY["projtape"], 1),
    "verif": lambda m, maps: m.verif_off(),
    "qtape": lambda m, maps: m.qtape_off(),
}


def read_tape(names):
    return lambda m: dict(info=m.tape_info, steps=m.tape_steps().tolist(), times=m.tape_times(), data={n: host(m.tape(n)) for n in names})


def read_enstape(m):
    data = {}
    for n in cc.ENSTAPE:
        mean, std = m.enstape(n)
        data[n] = dict(mean=host(mean), std=host(std), m2=host(m.enstape_moments(n)[2]))
    return dict(info=m.enstape_info, steps=m.enstape_steps().tolist(), times=m.enstape_times(), data=data)


def read_verif(m):
    got = m.verif()
    return dict(info=m.verif_info(), steps=m.verif_steps().tolist(), times=m.verif_times(),
                scores=np.stack([host(got[k]) for k in vref.NAMES], axis=-1), rmse=host(got["rmse"]), spread=host(got["spread"]),
                analysis=host(got["analysis"]), hist=host(m.verif_hist()))


READ = {
    "stats": lambda m: dict(samples=m.stats_samples, mean={n: host(m.stats_mean(n)) for n in cc.STATS},
                            var={n: host(m.stats_var(n)) for n in cc.STATS}),
    "tape": read_tape(cc.TAPED),
    "derive": read_tape(cc.DERIVE_TAPED),
    "plev": read_tape(cc.PLEV_TAPED),
    "spectra": lambda m: dict(info=m.spectra_info(), steps=m.spectra_steps().tolist(), times=m.spectra_times(),
                              data={n: host(m.spectra(n)) for n in cc.SPECTRA}),
    "enstape": read_enstape,
    "acctape": lambda m: dict(info=m.acctape_info, steps=m.acctape_steps().tolist(), times=m.acctape_times(),
                              counts=m.acctape_counts().tolist(), data={"%s %s" % e: host(m.acctape(*e)) for e in cc.ACCTAPE}),
    "wintape": lambda m: dict(info=m.wintape_info, steps=m.wintape_steps().tolist(), times=m.wintape_times(),
                              counts=[c.tolist() for c in m.wintape_counts()],
                              data={"%s %s" % e[:2]: host(m.wintape(*e[:2])) for e in cc.WINTAPE}),
    "projtape": lambda m: dict(info=m.projtape_info, steps=m.projtape_steps().tolist(), times=m.projtape_times(), data=host(m.projtape())),
    "verif": read_verif,
    "qtape": lambda m: dict(info=m.qtape_info(), steps=m.qtape_steps().tolist(), times=m.qtape_times(),
                            planes=np.stack([host(m.qtape(k)) for k in range(len(cc.QTAPE))], axis=1)),
}


def read_drivers(m, driver):
    out = dict(nudge=m.nudge_info())
    if driver == "A":
        got = m.breed()
        out["breed"] = dict(info=m.breed_info(), steps=m.breed_steps().tolist(), times=m.breed_times(), amplitude=host(got["amplitude"]),
                            factor=host(got["factor"]), growth=m.breed_growth(), gram=host(m.breed_gram()))
    elif driver == "B":
        got, last = m.assim(), m.assim_weights()
        out["assim"] = dict(info=m.assim_info(), steps=m.assim_steps().tolist(), times=m.assim_times(),
                            stats=np.stack([host(got[k]) for k in ("mean", "variance", "innovation", "used")], axis=-1),
                            W=host(last["W"]), Y=host(last["Y"]))
    return out


def mismatches(got, want, path=""):
    """the paths at which two nested results differ: arrays by shape, dtype and bits, everything else by =="""
    if isinstance(want, dict):
        assert isinstance(got, dict) and got.keys() == want.keys(), path
        return [p for k in want for p in mismatches(got[k], want[k], "%s/%s" % (path, k))]
    if isinstance(want, np.ndarray):
        COMPARED[0] += 1
        same = got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))
        return [] if same else [path]
    return [] if got == want else [path]


def check_schedule(rings, driver, start, stop):
    """assertion 4: the stamps and counters of every ring in `rings` against the Python schedule"""
    for name, ring in rings.items():
        if name == "stats":
            assert ring["samples"] == len(cc.due(cc.EVERY["stats"], start, stop)), ring["samples"]
            continue
        key = "tape" if name in ("derive", "plev") else name
        every = cc.ring_steps(key, driver, start, stop)
        want = cc.held(every, key)
        assert ring["steps"] == want, (name, ring["steps"], want)
        assert (ring["info"]["taken"], ring["info"]["held"]) == (len(every), len(want)), (name, ring["info"])
        assert len(ring["times"]) == len(want) and all(a < b for a, b in zip(ring["times"], ring["times"][1:])), name
    if "acctape" in rings:
        rows, _ = cc.window_rows(cc.EVERY["acctape"], start, stop)
        assert rings["acctape"]["counts"] == [r[2] for r in cc.held(rows, "acctape")]
    if "wintape" in rings:
        rows, _ = cc.window_rows(cc.EVERY["wintape"], start, stop, cc.WIN_SAMPLE_EVERY)
        assert rings["wintape"]["counts"] == [[r[1] for r in cc.held(rows, "wintape")], [r[2] for r in cc.held(rows, "wintape")]]
    if "verif" in rings:
        want = [1 if "verif1" in cc.events_at(s, driver) else 0 for s in rings["verif"]["steps"]]
        assert rings["verif"]["analysis"].tolist() == want, (rings["verif"]["analysis"], want)


def snapshot(model):
    """what an fp64 tape would hold of the state as it stands, for the planes the verification's entries name (as
    tests/test_verif_gpu.py's: the grid arrays brought up to date, the pressure-level and derived kernels on them)"""
    model.spectral2grid()
    computed = dict(model.plev(["z_plev", "mslp"], refresh=False))
    computed.update(model.derived(["tcwv"], refresh=False))
    out = {}
    for name, level, _ in cc.VERIF:
        x = computed[name] if name in computed else model.device_view(name).double()
        out[(name, level)] = host(x[:, level] if x.dim() == 4 else x).copy()
    return out


def observations(Y, k):
    """From an observation-space ensemble [E][r]: observations 0.7 prior standard deviations off the prior mean, to alternating
    sides, with error variances equal to the prior variances; entry 1 of the second row is missing."""
    mean, var = Y.mean(axis=1), Y.var(axis=1, ddof=1)
    yo = mean + 0.7 * np.sqrt(var) * np.where(np.arange(len(mean)) % 2 == 0, 1.0, -1.0)
    if k == 1:
        yo[1] = np.nan
    return yo, np.where(var > 0.0, var, 1.0)


class Crowd:
    """The models of one (plan, driver) and what they handed out, kept for the tests below."""

    def __init__(self, spectral, bc, maps, plan_key, driver, consumers=cc.CONSUMERS, calls=cc.CALLS, checked=True, switch_off=True):
        from pyspeedy_amd import nudge_gains
        from pyspeedy_amd.model import EnsembleModel
        t0 = time.perf_counter()
        plan = self.plan = cc.PLANS[plan_key]
        self.key, self.driver, self.maps, self.models = plan_key, driver, maps, []
        self.consumers, self.calls, self.stop = consumers, calls, cc.START + sum(calls)
        M = plan["members"]

        def fresh():
            model = EnsembleModel(spectral, M)
            self.models.append(model)
            model.set_bc(bc)
            for name, value in plan["options"]:
                model.set_option(name, value)
            if plan["fp32"]:
                model.set_physics_precision(True)
            perturb(model)
            model.plev_configure(cc.LEVELS_HPA)
            model.run(cc.START)
            return model

        still = fresh()
        base = still.get("t", 0)[..., 0]
        rng = np.random.default_rng(77)
        targets = np.stack([base * (1.0 + 2e-3 * rng.standard_normal(base.shape)) for _ in cc.NUDGE_STAMPS])
        if driver == "A":  # the target amplitude: half of what the first bred member has at the start
            control = np.asarray(plan["control"], dtype=np.int32)
            still.breed_configure(control, 1.0, cc.DRIVER_EVERY, weights="total_energy", capacity=1, in_loop=False)
            amplitude = float(host(still.breed_amplitude())[int(np.flatnonzero(control >= 0)[0])])
            still.breed_off()
            assert amplitude > 0

        def nudged():
            model = fresh()
            model.nudge_configure({"t": nudge_gains(6.0)}, capacity=len(cc.NUDGE_STAMPS))
            model.nudge_targets(cc.NUDGE_STAMPS, {"t": targets})
            return model

        self.table, self.after = [], {}
        if driver == "B":  # the host loop run(k); assim_apply(): it makes the observations from its own priors, and keeps the
            # planes its analyses left at the steps where the verification is due as well
            loop = nudged()
            loop.assim_configure(maps, cc.ASSIM, plan["assim"], cc.DRIVER_EVERY, capacity=8, inflation=cc.INFLATION, in_loop=False)
            for step in cc.ROWS:
                loop.run(step - loop.current_step)
                self.table.append(observations(host(loop.assim_compute()), len(self.table)))
                loop.assim_observations(cc.ROWS[:len(self.table)], np.stack([t[0] for t in self.table]), np.stack([t[1] for t in self.table]))
                loop.assim_apply()
                if step % cc.VERIF_EVERY == 0:
                    self.after[step] = snapshot(loop)
            assert loop.assim_info()["applied"] == len(cc.ROWS)

        def driven():
            model = nudged()
            if driver == "A":
                model.breed_configure(control, 0.5 * amplitude, cc.DRIVER_EVERY, weights="total_energy", capacity=cc.CAPACITY["breed"],
                                      orthogonalize=True)
            elif driver == "B":
                model.assim_configure(maps, cc.ASSIM, plan["assim"], cc.DRIVER_EVERY, capacity=cc.CAPACITY["assim"], inflation=cc.INFLATION)
                model.assim_observations(cc.ROWS, np.stack([t[0] for t in self.table]), np.stack([t[1] for t in self.table]))
            return model

        def crowded():
            model = driven()
            for name in consumers:
                if name not in ("derive", "plev"):  # (the crowd's tape names their variables among the others)
                    CONFIGURE[name](model, plan, maps)
            return model

        bare, crowd = driven(), crowded()
        solo = {}
        for name in consumers:
            solo[name] = driven()
            CONFIGURE[name](solo[name], plan, maps)
        for model in [still, bare, crowd] + list(solo.values()):
            for k in calls:
                model.run(k)
        self.config, self.rim = crowd.config(), crowd.get_option("quiet_rim_members")
        self.views = {n: crowd.device_view(n).dtype for n in ("precnv", "precls")}
        self.reg = dict(still=registry(still), bare=registry(bare), crowd=registry(crowd))
        self.rings = dict(crowd={name: READ[name](crowd) for name in consumers})
        self.solo = {name: READ[name](solo[name]) for name in consumers}
        self.drivers = dict(bare=read_drivers(bare, driver), crowd=read_drivers(crowd, driver))
        self.solo_state = {name: differing({n: [solo[name].get(n, i) for i in range(M)] for n in SPEC},
                                           {n: self.reg["bare"][n] for n in SPEC}) for name in consumers}
        if checked:
            again = crowded()
            self.codes = [again.run_checked(k)[0] for k in calls]
            self.reg["checked"] = registry(again)
            self.rings["checked"] = {name: READ[name](again) for name in consumers}
            self.drivers["checked"] = read_drivers(again, driver)
            again.close()
        self.models_run, self.t_main = len(self.models), time.perf_counter() - t0
        # 7: one consumer after the other goes off in the crowd; the others continue as their solo models do
        self.rounds, live, stop = [], [n for n in cc.OFF_ORDER if n in consumers], self.stop
        if switch_off:
            for name in list(live):
                OFF[name](crowd, maps)
                live.remove(name)
                for model in [crowd, bare] + [solo[k] for k in live]:
                    model.run(cc.EXTRA)
                stop += cc.EXTRA
                got = {k: READ[k](crowd) for k in live}
                bad = [p for k in live for p in mismatches(got[k], READ[k](solo[k]), k)]
                self.rounds.append(dict(off=name, live=tuple(live), stop=stop, rings=got, bad=bad, drivers=read_drivers(crowd, driver),
                                        drivers_bare=read_drivers(bare, driver)))
            self.reg["crowd_end"], self.reg["bare_end"] = registry(crowd), registry(bare)
        self.t_all = time.perf_counter() - t0
        WALL[(plan_key, driver, len(consumers))] = (self.models_run, self.t_main, self.t_all)

    def planes(self, step):
        """{(name, level): [M][48][96]} of the crowd's own fp64 tape behind `step`"""
        tape = self.rings["crowd"]["tape"]
        t = tape["steps"].index(step)
        out = {}
        for entries in (cc.PROJTAPE, cc.VERIF, cc.QTAPE):
            for name, level in (e[:2] for e in entries):
                x = tape["data"][name][:, t]
                out[(name, level)] = x[:, level] if x.ndim == 4 else x
        return out

    def close(self):
        for model in self.models:
            model.close()


@pytest.fixture(scope="module", params=cc.CASES, ids=["%s-%s" % c for c in cc.CASES])
def crowd(request, spectral, bc, maps):
    c = Crowd(spectral, bc, maps, *request.param)
    yield c
    c.close()
    print("\n%s driver %s: %d models, %.1f s to the rings, %.1f s with the switch-off rounds; %d arrays compared so far"
          % (c.key, c.driver, c.models_run, c.t_main, c.t_all, COMPARED[0]))


# ---- the plan is the one the case is about ---------------------------------------------------------------------------------------------
def test_the_plan_is_the_one_the_case_is_about(crowd):
    cfg = crowd.config
    if crowd.key == "serial_5":
        assert (cfg["chunks"], cfg["rounds"]) == (1, 1) and not cfg["physics_storage32"]
    elif crowd.key == "groups_rounds_12":
        assert (cfg["chunks"], cfg["rounds"], cfg["tau_recompute"]) == (2, 3, 2) and crowd.rim >= 0 and not cfg["physics_storage32"]
    else:
        import torch
        assert cfg["physics_storage32"] and cfg["chunks"] == 2
        assert crowd.views == {"precnv": torch.float32, "precls": torch.float32}
    if crowd.key != "fp32_storage_6":
        import torch
        assert crowd.views == {"precnv": torch.float64, "precls": torch.float64}


# ---- 1: the state ----------------------------------------------------------------------------------------------------------------------
def test_the_crowd_leaves_the_state_of_the_drivers_alone(crowd):
    assert differing(crowd.reg["crowd"], crowd.reg["bare"]) == []
    assert differing(crowd.reg["checked"], crowd.reg["bare"]) == []
    assert all((codes == -1).all() for codes in crowd.codes), crowd.codes
    assert all(bad == [] for bad in crowd.solo_state.values()), crowd.solo_state  # (nor does any consumer alone move it)
    # the drivers acted: every prognostic variable of every member (all are nudged) differs from the run without them
    moved = differing({n: crowd.reg["crowd"][n] for n in SPEC}, {n: crowd.reg["still"][n] for n in SPEC})
    assert sorted(moved) == sorted((n, i) for n in SPEC for i in range(crowd.plan["members"]))


# ---- 2: every consumer's ring ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.CONSUMERS)
def test_a_consumers_ring_in_the_crowd_is_the_one_it_holds_alone(crowd, name):
    assert mismatches(crowd.rings["crowd"][name], crowd.solo[name], name) == []
    assert mismatches(crowd.rings["checked"][name], crowd.rings["crowd"][name], name) == []


# ---- 3: the drivers' rings ---------------------------------------------------------------------------------------------------------------
def test_the_drivers_rings_are_those_of_the_run_without_consumers(crowd):
    assert mismatches(crowd.drivers["crowd"], crowd.drivers["bare"], "drivers") == []
    assert mismatches(crowd.drivers["checked"], crowd.drivers["bare"], "drivers") == []
    got = crowd.drivers["crowd"]
    assert got["nudge"]["applied"] == crowd.stop - cc.START and got["nudge"]["in_loop"]
    if crowd.driver == "A":
        ring = got["breed"]
        assert ring["steps"] == cc.held(cc.ring_steps("breed"), "breed") and ring["info"]["applied"] == len(cc.ring_steps("breed"))
        assert ring["info"]["orthogonalize"] and ring["info"]["families"] == 2 and ring["info"]["largest_family"] == 2
        bred = [i for i, c in enumerate(crowd.plan["control"]) if c >= 0]
        assert (ring["amplitude"][:, bred] > 0).all() and np.isfinite(ring["growth"][1:, bred]).all()
        assert (np.diag(ring["gram"])[bred] > 0).all() and np.count_nonzero(np.diag(ring["gram"])) == len(bred)
    else:
        ring = got["assim"]
        events = cc.due(cc.DRIVER_EVERY, cc.START, crowd.stop)
        assert ring["steps"] == cc.held(list(cc.ROWS), "assim")
        assert (ring["info"]["applied"], ring["info"]["skipped"]) == (len(cc.ROWS), len(events) - len(cc.ROWS))
        used = ring["stats"][:, :, 3]
        assert used[-1].all() and used[0].tolist() == [1.0, 0.0, 1.0, 1.0]  # (the held events: 42 with its missing entry, 72)


# ---- 4: the schedule -----------------------------------------------------------------------------------------------------------------------
def test_every_rings_stamps_are_the_python_schedules(crowd):
    check_schedule(crowd.rings["crowd"], crowd.driver, cc.START, crowd.stop)
    check_schedule(crowd.solo, crowd.driver, cc.START, crowd.stop)
    for name in cc.SMALL:
        if name in crowd.rings["crowd"]:
            assert crowd.rings["crowd"][name]["info"]["taken"] > cc.CAPACITY[name], name  # (it wrapped)


# ---- 5: anchors on the crowd's own tape ----------------------------------------------------------------------------------------------------
def test_the_projection_rows_are_the_arbiters_on_the_crowds_tape(crowd):
    ring = crowd.rings["crowd"]["projtape"]
    assert ring["data"].shape == (crowd.plan["members"], cc.CAPACITY["projtape"], len(cc.PROJTAPE))
    for j, step in enumerate(ring["steps"]):
        planes = crowd.planes(step)
        for e, (name, level, pattern) in enumerate(cc.PROJTAPE):
            want = proj.project(crowd.maps[pattern], planes[(name, level)])
            assert np.array_equal(bits(ring["data"][:, j, e]), bits(want)), (step, name, level)


def test_the_verification_rows_are_the_arbiters_in_both_phases(crowd):
    ring = crowd.rings["crowd"]["verif"]
    mask, truth = crowd.plan["verif"]
    members = cc.masked(mask)
    r = len(members)
    assert ring["scores"].shape == (cc.CAPACITY["verif"], 2, len(cc.VERIF), 4) and ring["hist"].shape[-1] == r + 2
    filled = 0
    for j, step in enumerate(ring["steps"]):
        want, want_hist = vref.event(crowd.planes(step), truth, members, cc.VERIF, crowd.maps)
        got = ring["scores"][j, 0]
        assert np.array_equal(bits(got), bits(want)), (step, int((bits(got) != bits(want)).sum()))
        assert np.array_equal(ring["hist"][j, 0], want_hist[:, :r + 2]), step
        if "verif1" in cc.events_at(step, crowd.driver):  # the arbiter on the state the host loop's analysis left
            want, want_hist = vref.event(crowd.after[step], truth, members, cc.VERIF, crowd.maps)
            got = ring["scores"][j, 1]
            assert np.array_equal(bits(got), bits(want)), (step, int((bits(got) != bits(want)).sum()))
            assert np.array_equal(ring["hist"][j, 1], want_hist[:, :r + 2]), step
            assert not np.array_equal(bits(got[0]), bits(ring["scores"][j, 0, 0]))  # (the analysis moved the temperature's scores)
            filled += 1
        else:
            assert np.isnan(ring["scores"][j, 1]).all() and (ring["hist"][j, 1] == -1).all(), step
    assert filled == (1 if crowd.driver == "B" else 0)
    # precnv (a float plane under fp32 storage): it rains somewhere, its dry points are ties, and no two events agree
    wet = ring["scores"][:, 0, cc.VERIF_PRECNV]
    assert np.isfinite(wet).all() and wet[:, 1:].all() and len({bits(row).tobytes() for row in wet}) == len(wet)
    assert (ring["hist"][:, 0, cc.VERIF_PRECNV, r + 1] > 0).all()


def test_the_quantile_planes_are_the_arbiters_on_the_crowds_tape(crowd):
    ring = crowd.rings["crowd"]["qtape"]
    members = cc.masked(crowd.plan["qtape"])
    assert ring["planes"].shape == (cc.CAPACITY["qtape"], len(cc.QTAPE), 48, 96)
    for j, step in enumerate(ring["steps"]):
        want = qref.event(crowd.planes(step), members, cc.QTAPE)
        for k in range(len(cc.QTAPE)):
            got = ring["planes"][j, k]
            assert np.array_equal(bits(got), bits(want[k])), (step, k, int((bits(got) != bits(want[k])).sum()))
    wet, wet90 = ring["planes"][:, cc.QTAPE_PRECNV], ring["planes"][:, cc.QTAPE_PRECNV_Q]
    assert wet.any(axis=(1, 2)).all() and (wet == 0.0).any() and wet90.any()
    assert len({bits(p).tobytes() for p in wet90}) > 1  # (the quantile of precnv differs between events)
    for name in ("precnv", "precls"):  # the tape the arbiters read holds rain
        assert crowd.rings["crowd"]["tape"]["data"][name].any(), name


# ---- 7: one consumer after the other switched off ------------------------------------------------------------------------------------------
def test_switching_consumers_off_one_by_one_leaves_the_others_and_the_state_alone(crowd):
    assert [r["off"] for r in crowd.rounds] == list(cc.OFF_ORDER)
    for r in crowd.rounds:
        assert r["bad"] == [], (r["off"], r["bad"])
        check_schedule(r["rings"], crowd.driver, cc.START, r["stop"])
        assert mismatches(r["drivers"], r["drivers_bare"], "drivers behind %s_off" % r["off"]) == []
    assert crowd.rounds[-1]["live"] == () and crowd.rounds[0]["stop"] == crowd.stop + cc.EXTRA
    # the windows that were open across the first switch: closed with the counts the schedule gives them
    first = crowd.rounds[0]["rings"]
    assert first["acctape"]["steps"][-2:] == [80, 84] and first["acctape"]["counts"][-2:] == [4, 4]
    assert first["wintape"]["steps"][-1] == 84 and [c[-1] for c in first["wintape"]["counts"]] == [3, 6]
    assert differing(crowd.reg["crowd_end"], crowd.reg["bare_end"]) == []


# ---- 6: nine recorders and nudging, no joined consumer: one segment of 40 steps ----------------------------------------------------------
@pytest.fixture(scope="module")
def recorders_only(spectral, bc, maps):
    c = Crowd(spectral, bc, maps, "groups_rounds_12", None, consumers=cc.RECORDERS, calls=(cc.SOLO_CALL,), switch_off=False)
    yield c
    c.close()
    print("\nrecorders only: %d models, %.1f s; %d arrays compared in the module" % (c.models_run, c.t_all, COMPARED[0]))


def test_nine_recorders_in_one_long_segment(recorders_only):
    c = recorders_only
    assert (c.config["chunks"], c.config["rounds"], c.config["tau_recompute"]) == (2, 3, 2) and c.rim >= 0
    assert cc.segments(cc.START, c.calls, ()) == [(cc.START, cc.SOLO_CALL)]
    assert differing(c.reg["crowd"], c.reg["bare"]) == [] and differing(c.reg["checked"], c.reg["bare"]) == []
    assert all((codes == -1).all() for codes in c.codes)
    for name in cc.RECORDERS:
        assert mismatches(c.rings["crowd"][name], c.solo[name], name) == [], name
        assert mismatches(c.rings["checked"][name], c.rings["crowd"][name], name) == [], name
    assert mismatches(c.drivers["crowd"], c.drivers["bare"], "nudge") == [] and c.drivers["crowd"]["nudge"]["applied"] == cc.SOLO_CALL
    check_schedule(c.rings["crowd"], None, cc.START, c.stop)
    for name in ("spectra", "enstape", "acctape", "wintape", "projtape"):
        assert c.rings["crowd"][name]["info"]["taken"] > cc.CAPACITY[name], name
    moved = differing({n: c.reg["crowd"][n] for n in SPEC}, {n: c.reg["still"][n] for n in SPEC})
    assert sorted(moved) == sorted((n, i) for n in SPEC for i in range(c.plan["members"]))
