"""GPU tier: the quantile tape (spd_model_qtape_*, csrc/qtape.hip) against its definition restated in numpy
(tests/qtape_reference.py; include/pyspeedy_amd.h).  Every plane is compared as bit patterns with the arbiter
applied to the fp64 tape of a twin model sampled at the same steps.

Shapes: 5 members with the masks r = 4 and r = 3; 8 members in 2 member groups and 2 rounds, member 3 unused and member 6 left out
(r = 6); 66 members, r = 64, one qtape_apply only (the full LDS column and member indices beyond 63).

Ten entries: t_grid at the lowest level (min, max, median), u_grid level 0 (q = 0.1, 0.9), mslp prob_below a threshold that is
the twin's own ensemble median at one point of its first sample, z_plev at 500 hPa (q = 1/3), precnv (prob_above 0 and q = 0.9: its
dry points tie at zero), tcwv (median).

  1  every = 3 over calls of 5, 1, 7 and 12 steps from step 30: in-loop (a ring of 5 that wraps), the host loop run(k);
     qtape_compute(); qtape_apply() (a ring of 16), checked calls: the same bits and stamps in all of them
  2  isolation: every registry variable is bitwise that of a model without any recorder; a verification tape (every 2) and a
     projection tape beside it hold the bits they hold alone
  3  66 members, one qtape_apply
  4  an unperturbed ensemble: min = max = every quantile = the member's tape value
  5  beside in-loop assimilation (tests/test_assim_gpu.py's 8-member shape, rows at 32 and 40): the sample is the arbiter on the
     state before the analysis; states and the assimilation's ring are those of the run without the quantile tape
  6  lifecycle and refusals with a model
"""
import ctypes as C

import numpy as np
import pytest

import qtape_reference as ref
from test_breed_gpu import bc, bits, differing, perturb, registry  # noqa: F401

pytestmark = pytest.mark.gpu

START, EVERY, CALLS = 30, 3, (5, 1, 7, 12)  # (the first convective rain falls around step 24)
EVENTS = [s for s in range(START + 1, START + sum(CALLS) + 1) if s % EVERY == 0]  # 33, 36, ..., 54
# (members, options, mask of the quantile tape, truth of the verification tape beside it)
SHAPES = {"5_members_r4": (5, (), (1, 1, 0, 1, 1), 2),
          "5_members_r3": (5, (), (1, 1, 0, 1, 0), 2),
          "8_members_2_groups_2_rounds": (8, (("member_groups", 2), ("block_members", 2)), (1, 1, 1, 0, 1, 1, 0, 1), 6)}
POINT = (30, 17)  # (row, column) whose ensemble median of mslp is the threshold
MSLP, WET, WET90 = 5, 7, 8
TAPED = ("t_grid", "u_grid", "mslp", "z_plev", "precnv", "tcwv")
VERIF_ENTRIES = (("t_grid", 7, 0), ("mslp", 0, 0), ("precnv", 0, 0))
VERIF_EVERY, PROJ_EVERY = 2, 2


def entries_for(threshold):
    return (("t_grid", 7, "min"), ("t_grid", 7, "max"), ("t_grid", 7, "quantile", 0.5), ("u_grid", 0, "quantile", 0.1),
            ("u_grid", 0, "quantile", 0.9), ("mslp", 0, "prob_below", threshold), ("z_plev", 0, "quantile", 1.0 / 3.0),
            ("precnv", 0, "prob_above", 0.0), ("precnv", 0, "quantile", 0.9), ("tcwv", 0, "quantile", 0.5))


@pytest.fixture(scope="module")
def maps():
    import pyspeedy_amd
    return np.stack([pyspeedy_amd.projection_weights().global_mean()])


def fresh(spectral, bc, members, options=(), perturbed=True):
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, members)
    model.set_bc(bc)
    for name, value in options:
        model.set_option(name, value)
    if perturbed:
        perturb(model)
    model.plev_configure([500.0])
    model.run(START)
    return model


def tape_planes(model, t):
    """{(name, level): [M][48][96]} of sample t of the model's fp64 tape, for the planes the entries name"""
    out = {}
    for name, level in (("t_grid", 7), ("u_grid", 0), ("mslp", 0), ("z_plev", 0), ("precnv", 0), ("tcwv", 0)):
        x = model.tape(name, t0=t, nt=1)[:, 0].cpu().numpy()
        assert x.dtype == np.float64
        out[(name, level)] = x[:, level] if x.ndim == 4 else x
    return out


def ring_of(model):
    n = len(model.qtape_entries)
    return dict(planes=np.stack([model.qtape(k).cpu().numpy() for k in range(n)], axis=1), steps=model.qtape_steps().tolist(),
                times=model.qtape_times())


def same_rows(ring, first, want):
    """the ring's events from event `first` on are the arbiter's"""
    n = len(ring["steps"])
    assert ring["planes"].shape == (n, want[0].shape[0], 48, 96)
    for t in range(n):
        for k in range(want[0].shape[0]):
            got, exp = bits(ring["planes"][t, k]), bits(want[first + t][k])
            assert np.array_equal(got, exp), (t, k, int((got != exp).sum()))


def verif_ring(model):
    got = model.verif()
    return [got[k].cpu().numpy() for k in ("bias", "mse", "variance", "crps")] + [model.verif_hist().cpu().numpy(), model.verif_steps()]


class Plans:
    """The runs of one ensemble shape from step 30, each on a model of its own."""

    def __init__(self, spectral, bc, maps, members, options, mask, truth):
        self.members, self.mask, self.models = members, mask, []
        self.masked = [i for i in range(members) if mask[i]]
        vmask = [1 if mask[i] and i != truth else 0 for i in range(members)]

        def start():
            model = fresh(spectral, bc, members, options)
            self.models.append(model)
            return model

        # the twin: an fp64 tape, a verification tape and a projection tape, no quantile tape
        twin = start()
        twin.tape_configure(TAPED, EVERY, len(EVENTS), dtype="float64")
        twin.verif_configure(maps, VERIF_ENTRIES, vmask, truth, VERIF_EVERY, capacity=16)
        twin.projtape_configure(maps, VERIF_ENTRIES, PROJ_EVERY, 16)
        for k in CALLS:
            twin.run(k)
        assert twin.tape_steps().tolist() == EVENTS
        planes = [tape_planes(twin, t) for t in range(len(EVENTS))]
        self.threshold = float(np.median(planes[0][("mslp", 0)][self.masked][:, POINT[0], POINT[1]]))
        self.entries = entries_for(self.threshold)
        self.want = [ref.event(p, self.masked, self.entries) for p in planes]
        self.verif_twin, self.proj_twin, self.times_twin = verif_ring(twin), twin.projtape().cpu().numpy(), twin.tape_times()
        # in the loop, beside a verification tape and a projection tape; the ring wraps
        a = start()
        a.qtape_configure(self.entries, mask, EVERY, capacity=5)
        a.verif_configure(maps, VERIF_ENTRIES, vmask, truth, VERIF_EVERY, capacity=16)
        a.projtape_configure(maps, VERIF_ENTRIES, PROJ_EVERY, 16)
        self.info0, self.entries_a = a.qtape_info(), a.qtape_entries
        for k in CALLS:
            a.run(k)
        self.a, self.ring_a, self.info_a = registry(a), ring_of(a), a.qtape_info()
        self.verif_a, self.proj_a = verif_ring(a), a.projtape().cpu().numpy()
        never = start()
        for k in CALLS:
            never.run(k)
        self.never = registry(never)
        # the host loop; qtape_compute() in front of every qtape_apply()
        b, self.computed = start(), []
        b.qtape_configure(self.entries, mask, EVERY, capacity=16, in_loop=False)
        for k in CALLS:
            left = k
            while left:
                n = min(EVERY - b.current_step % EVERY, left)
                b.run(n)
                left -= n
                if b.current_step % EVERY == 0:
                    self.computed.append(b.qtape_compute().cpu().numpy())
                    b.qtape_apply()
        self.b, self.ring_b, self.info_b = registry(b), ring_of(b), b.qtape_info()
        checked = start()
        checked.qtape_configure(self.entries, mask, EVERY, capacity=16)
        self.codes = [checked.run_checked(k)[0] for k in CALLS]
        self.checked, self.ring_checked = registry(checked), ring_of(checked)
        # in_loop = False and no qtape_apply: nothing is recorded
        idle = start()
        idle.qtape_configure(self.entries, mask, EVERY, capacity=4, in_loop=False)
        idle.run(CALLS[0] + CALLS[1])
        self.info_idle = idle.qtape_info()
        idle.qtape_off()
        self.info_off, self.entries_off = idle.qtape_info(), idle.qtape_entries

    def close(self):
        for model in self.models:
            model.close()


@pytest.fixture(scope="module", params=list(SHAPES))
def plans(request, spectral, bc, maps):
    p = Plans(spectral, bc, maps, *SHAPES[request.param])
    yield p
    p.close()


# ---- 1: the schedule and the arithmetic ----------------------------------------------------------------------------------------
def test_in_loop_planes_are_the_arbiters_on_the_twins_tape(plans):
    r = len(plans.masked)
    assert plans.info0 == dict(members=r, entries=len(plans.entries), every=EVERY, capacity=5, taken=0, held=0, in_loop=True, applied=0)
    assert plans.entries_a == tuple((e + (0.0,))[:4] for e in plans.entries)
    assert (plans.info_a["taken"], plans.info_a["held"], plans.info_a["applied"]) == (len(EVENTS), 5, len(EVENTS))
    assert plans.ring_a["steps"] == EVENTS[-5:] and plans.ring_a["times"] == plans.times_twin[-5:]  # (the ring wrapped)
    same_rows(plans.ring_a, len(EVENTS) - 5, plans.want)
    if plans.members == 8:
        assert (plans.models[0].config()["chunks"], plans.models[0].config()["rounds"]) == (2, 2)


def test_the_arbiters_planes_vary_and_both_outcomes_occur(plans):
    r = len(plans.masked)
    want = np.stack(plans.want)  # [T][E][48][96]
    assert np.isfinite(want).all()
    for k in range(want.shape[1]):
        assert len({bits(want[t, k]).tobytes() for t in range(len(EVENTS))}) == len(EVENTS), k  # no two events alike
    assert (want[:, 0] < want[:, 1]).all() and (want[:, 0] <= want[:, 2]).all() and (want[:, 2] <= want[:, 1]).all()  # members differ
    assert (want[:, 3] <= want[:, 4]).all() and (want[:, 3] < want[:, 4]).any()
    # the shares are multiples of 1 / r; at the chosen point of the first sample the threshold is the median: members on both sides
    for k in (MSLP, WET):
        assert np.array_equal(np.rint(want[:, k] * r) / r, want[:, k])
    at = want[0, MSLP, POINT[0], POINT[1]]
    assert 0.0 < at < 1.0 and (want[:, MSLP] == 0.0).any() and (want[:, MSLP] == 1.0).any()
    # convective rain: dry points in every member (probability 0, and a 0.9 quantile of exactly zero among tied zeros) and wet ones
    wet = want[:, WET]
    assert (wet == 0.0).any(axis=(1, 2)).all() and (wet > 0.0).any(axis=(1, 2)).all() and (wet == 1.0).any()
    assert (want[:, WET90][wet == 0.0] == 0.0).all() and (want[:, WET90] > 0.0).any()
    got = plans.ring_a["planes"][:, WET]
    assert (got == 0.0).any() and (got > 0.0).any()


def test_in_loop_is_the_host_loop_and_the_checked_call(plans):
    assert plans.ring_b["steps"] == plans.ring_checked["steps"] == EVENTS  # (these rings do not wrap)
    same_rows(plans.ring_b, 0, plans.want)
    same_rows(plans.ring_checked, 0, plans.want)
    assert plans.ring_b["times"] == plans.ring_checked["times"] == plans.times_twin
    for t, planes in enumerate(plans.computed):  # qtape_compute() in front of each qtape_apply()
        assert np.array_equal(bits(planes), bits(plans.want[t])), t
    assert len(plans.computed) == len(EVENTS) and plans.info_b["taken"] == len(EVENTS) and not plans.info_b["in_loop"]
    assert all((codes == -1).all() for codes in plans.codes)
    assert plans.info_idle["taken"] == 0 and plans.info_idle["members"] == len(plans.masked)
    assert plans.info_off == dict(members=0, entries=0, every=0, capacity=0, taken=0, held=0, in_loop=False, applied=0)
    assert plans.entries_off == ()


# ---- 2: isolation -----------------------------------------------------------------------------------------------------------
def test_the_recorder_changes_no_state_bit_and_no_other_ring(plans):
    assert differing(plans.a, plans.never) == []  # the extra cuts and the events move nothing
    assert differing(plans.b, plans.never) == [] and differing(plans.checked, plans.never) == []
    assert plans.proj_a.shape == plans.proj_twin.shape and plans.proj_a.shape[1] > 0
    assert np.array_equal(bits(plans.proj_a), bits(plans.proj_twin))
    assert plans.verif_a[-1].tolist() == plans.verif_twin[-1].tolist() and len(plans.verif_a[-1]) > len(EVENTS)
    for got, want in zip(plans.verif_a[:4], plans.verif_twin[:4]):
        assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(plans.verif_a[4], plans.verif_twin[4])


# ---- 3: the largest ensemble ------------------------------------------------------------------------------------------------
def test_sixty_four_members_in_one_apply(spectral, bc):
    members = 66
    mask = np.ones(members, dtype=np.int32)
    mask[[0, 40]] = 0
    masked = np.flatnonzero(mask).tolist()
    assert len(masked) == 64 and masked[-1] == 65
    twin, model = fresh(spectral, bc, members), fresh(spectral, bc, members)
    try:
        twin.tape_configure(TAPED, 3, 1, dtype="float64")
        twin.run(3)
        assert twin.tape_steps().tolist() == [START + 3]
        planes = tape_planes(twin, 0)
        entries = entries_for(float(np.median(planes[("mslp", 0)][masked][:, POINT[0], POINT[1]])))
        want = ref.event(planes, masked, entries)
        model.qtape_configure(entries, mask, 5, capacity=2, in_loop=False)
        assert model.qtape_info()["members"] == 64
        model.run(3)
        model.qtape_apply()
        ring = ring_of(model)
        assert ring["steps"] == [START + 3]
        same_rows(ring, 0, [want])
        assert np.array_equal(np.rint(want[MSLP] * 64) / 64, want[MSLP]) and 0.0 < want[MSLP][POINT] < 1.0
        assert len(np.unique(want[MSLP])) > 2 and (want[WET] == 0.0).any() and (want[WET] > 0.0).any()
        assert not np.array_equal(want[2], ref.event(planes, masked[:-2], entries)[2])  # (members 64 and 65 take part)
    finally:
        twin.close()
        model.close()


# ---- 4: an ensemble without a perturbation ----------------------------------------------------------------------------------
def test_identical_members_give_the_members_tape_value(spectral, bc):
    model = fresh(spectral, bc, 4, perturbed=False)
    try:
        qs = (0.0, 0.1, 1.0 / 3.0, 0.5, 0.9, 1.0)
        entries = [(n, lev, "min") for n, lev in (("t_grid", 7), ("precnv", 0), ("z_plev", 0))]
        entries += [(n, lev, "max") for n, lev in (("t_grid", 7), ("precnv", 0), ("z_plev", 0))]
        entries += [("t_grid", 7, "quantile", q) for q in qs] + [("precnv", 0, "quantile", q) for q in qs]
        entries += [("precnv", 0, "prob_above", 0.0), ("t_grid", 7, "prob_below", 280.0)]
        model.tape_configure(("t_grid", "precnv", "z_plev"), 3, 2, dtype="float64")
        model.qtape_configure(entries, (1, 1, 1, 1), 3, capacity=2)
        model.run(6)
        assert model.qtape_steps().tolist() == model.tape_steps().tolist() == [START + 3, START + 6]
        ring = ring_of(model)["planes"]
        for t in range(2):
            one = {"t_grid": model.tape("t_grid", t0=t, nt=1)[0, 0, 7].cpu().numpy(), "precnv": model.tape("precnv", t0=t, nt=1)[0, 0].cpu().numpy(),
                   "z_plev": model.tape("z_plev", t0=t, nt=1)[0, 0, 0].cpu().numpy()}
            for k, entry in enumerate(entries[:-2]):
                assert np.array_equal(bits(ring[t, k]), bits(one[entry[0]])), (t, entry)
            assert np.array_equal(ring[t, -2], (one["precnv"] > 0.0).astype(np.float64))
            assert np.array_equal(ring[t, -1], (one["t_grid"] < 280.0).astype(np.float64))
            assert 0 < ring[t, -2].sum() < 4608 and 0 < ring[t, -1].sum() < 4608
    finally:
        model.close()


# ---- 5: beside the in-loop assimilation -----------------------------------------------------------------------------------------
def test_beside_in_loop_assimilation_the_sample_is_the_state_before_the_analysis(spectral, bc):
    import test_assim_gpu as ta
    import test_verif_gpu as tv
    import pyspeedy_amd
    members, options, mask = ta.SHAPES["8_members_2_groups_2_rounds"]
    masked = [i for i in range(members) if mask[i]]
    pw = pyspeedy_amd.projection_weights()
    amaps = np.stack([pw.point(*ta.STATION), pw.box(150.0, -150.0, -40.0, 25.0), np.random.default_rng(2026).normal(0.0, 1.0, (48, 96)),
                      pw.global_mean(), np.zeros((48, 96))])
    entries = (("t_grid", 7, "min"), ("t_grid", 7, "quantile", 0.5), ("u_grid", 0, "quantile", 0.1), ("ps_grid", 0, "max"),
               ("mslp", 0, "prob_below", 101325.0), ("z_plev", 0, "quantile", 1.0 / 3.0), ("precnv", 0, "prob_above", 0.0))
    models = []

    def start(in_loop):
        model = ta.fresh(spectral, bc, members, options)
        models.append(model)
        views = {n: model.device_view(n) for n in ("t_grid", "u_grid", "ps_grid", "precnv")}
        model.assim_configure(amaps, ta.ENTRIES, mask, ta.EVERY, capacity=8, inflation=1.05, in_loop=in_loop)
        return model, views

    try:
        # the host loop without the quantile tape: observations from its own priors, the planes before every event
        host, views = start(False)
        table, before = [], {}
        while host.current_step < ta.START + ta.STEPS:
            host.run(min(ta.EVERY - host.current_step % ta.EVERY, ta.START + ta.STEPS - host.current_step))
            if host.current_step % ta.EVERY == 0:
                before[host.current_step] = tv.snapshot(host, views)
            if host.current_step in ta.ROWS:
                table.append(ta.observations(host.assim_compute().cpu().numpy()))
                host.assim_observations(ta.ROWS[:len(table)], np.stack([t[0] for t in table]), np.stack([t[1] for t in table]))
                host.assim_apply()
        events = sorted(before)
        assert events == [32, 36, 40]
        plain, _ = start(True)
        both, _ = start(True)
        both.qtape_configure(entries, mask, ta.EVERY, capacity=8)
        for model in (plain, both):
            model.assim_observations(ta.ROWS, np.stack([t[0] for t in table]), np.stack([t[1] for t in table]))
            model.run(ta.STEPS)
        ring = ring_of(both)
        assert ring["steps"] == events
        same_rows(ring, 0, [ref.event(before[step], masked, entries) for step in events])
        # states and the assimilation's ring are those of the run without the quantile tape, and of the host loop
        reg = registry(both)
        assert differing(reg, registry(plain)) == []
        # (the host loop's snapshots filled the registry's exported grid arrays, which a stepped model never writes)
        assert {n for n, _ in differing(reg, registry(host))} <= {"u_grid", "v_grid", "t_grid", "q_grid", "phi_grid", "ps_grid"}
        assert ta.same_ring(ta.ring_of(both), ta.ring_of(plain)) and ta.same_ring(ta.ring_of(both), ta.ring_of(host))
        assert both.assim_info() == plain.assim_info() and both.assim_info()["skipped"] == 1
    finally:
        for model in models:
            model.close()


# ---- 6: lifecycle and refusals that need a model --------------------------------------------------------------------------------
def test_refusals_and_lifecycle(spectral, bc):
    from pyspeedy_amd import SpeedyHipError
    from pyspeedy_amd.model import EnsembleModel
    model, other = EnsembleModel(spectral, 4), EnsembleModel(spectral, 4)
    entries = entries_for(101325.0)
    stored = tuple((e + (0.0,))[:4] for e in entries)
    everyone = (1, 1, 1, 1)
    try:
        model.set_bc(bc)
        perturb(model)
        with pytest.raises(SpeedyHipError, match="'mslp' needs target levels"):
            model.qtape_configure(entries, everyone, EVERY)
        model.plev_configure([500.0])
        for bad, message in (((1, 0, 0, 0), "1 members are masked in: the order statistics take 2 ... 64"),
                             ((1, 2, 0, 1), r"the mask of member 1 \(2\) is not 0 or 1")):
            with pytest.raises(SpeedyHipError, match=message):
                model.qtape_configure(entries, bad, EVERY)
        with pytest.raises(ValueError, match=r"one entry per member \(4\)"):
            model.qtape_configure(entries, (1, 1, 1), EVERY)
        for bad, message in (((("t_grid", 7, "quantile", 1.5),), "is not within 0 ... 1"),
                             ((("t_grid", 7, "quantile", float("nan")),), "is not within 0 ... 1"),
                             ((("mslp", 0, "prob_above", float("inf")),), "the threshold of entry 0 .'mslp'. is not finite"),
                             ((("t_grid", 8, "min"),), "level 8 of entry 0"),
                             ((("z_plev", 1, "min"),), r"level 1 of entry 0 \('z_plev'\) is out of range \(0 ... 0\)"),
                             ((("t_grid", 0, "min"),) * 65, "n_entries must be 1 ... 64, got 65"),
                             ((), "n_entries must be 1 ... 64, got 0")):
            with pytest.raises(SpeedyHipError, match=message):
                model.qtape_configure(bad, everyone, EVERY)
        with pytest.raises(ValueError, match="op must be one of"):
            model.qtape_configure((("t_grid", 0, "median"),), everyone, EVERY)
        with pytest.raises(ValueError, match="needs a parameter"):
            model.qtape_configure((("t_grid", 0, "quantile"),), everyone, EVERY)
        with pytest.raises(SpeedyHipError, match="every must be at least 1"):
            model.qtape_configure(entries, everyone, 0)
        with pytest.raises(SpeedyHipError, match="capacity must be at least 1"):
            model.qtape_configure(entries, everyone, EVERY, capacity=0)
        with pytest.raises(SpeedyHipError, match="no quantile tape configured"):
            model.qtape_apply()
        assert model.qtape_info()["members"] == 0 and model.qtape_entries == ()
        # an allocation that cannot succeed: the recorder is off, the byte count is told, the model steps on
        with pytest.raises(SpeedyHipError, match=r"cannot allocate the quantile tape \((\d{15,}) bytes asked for\); it is off"):
            model.qtape_configure(entries, everyone, EVERY, capacity=2 ** 31 - 1)
        assert model.qtape_info()["members"] == 0 and model.qtape_entries == ()
        model.qtape_configure(entries, everyone, EVERY, capacity=4)
        assert model.qtape_entries == stored
        # spd_model_copy_member does not carry the configuration
        other.set_bc(bc)
        other.copy_member_from(model, 0, 0)
        assert other.qtape_info()["members"] == 0 and other.qtape_entries == () and model.qtape_info()["members"] == 4
        with pytest.raises(SpeedyHipError, match="the quantile tape holds a pressure-level variable"):
            model.plev_configure([850.0])
        model.run(EVERY)
        assert model.qtape_steps().tolist() == [EVERY]
        with pytest.raises(SpeedyHipError, match=r"entry 10 is out of range \(0 ... 9\)"):
            model.qtape(len(entries))
        model.qtape_reset()
        assert model.qtape_info()["taken"] == 0 and model.qtape(0).shape == (0, 48, 96)
        with pytest.raises(SpeedyHipError, match="event range out of bounds"):
            model.qtape(0, 0, 1)
        # a checked call in flight
        stream = model._stream()
        assert model._lib.spd_model_step_checked_begin(model._m, EVERY, stream) == 0
        for call in (lambda: model.qtape(0), model.qtape_apply, model.qtape_compute, model.qtape_reset, model.qtape_off,
                     lambda: model.qtape_configure(entries, everyone, EVERY)):
            with pytest.raises(SpeedyHipError, match="in flight"):
                call()
        failed = np.zeros(4, dtype=np.int32)
        assert model._lib.spd_model_step_checked_end(model._m, failed.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
        assert failed.tolist() == [-1] * 4 and model.qtape_steps().tolist() == [2 * EVERY]
        # a member out of range: global-mean temperature of 500 K (diagnostics.f90:57-66), as tests/test_tape_gpu.py
        t = model.get("t", 1)
        t[0, 0, :, :] = 500.0 * np.sqrt(2.0)
        model.set("t", t, member=1)
        failed, _ = model.run_checked(EVERY)
        assert failed.tolist() == [-1, 0, -1, -1]
        with pytest.raises(SpeedyHipError, match="the quantile tape is invalid until spd_model_qtape_reset: member 1 failed the range check"):
            model.qtape(0)
        assert model.qtape_info()["taken"] == 2  # (the count is still told)
        model.qtape_reset()
        assert model.qtape(0).shape == (0, 48, 96)
        # spd_model_init: an empty ring, the configuration stays
        model.init((1982, 1, 1, 0, 0))
        model.run(EVERY)
        assert model.qtape_info()["taken"] == 1
        model.init((1982, 1, 1, 0, 0))
        assert model.qtape_info()["taken"] == 0 and model.qtape_info()["members"] == 4
    finally:
        model.close()
        other.close()


# an interleaved list that comes back to planes it has left (t_grid 7, z_plev 1 and precnv, not adjacent) and mixes sigma-level,
# pressure-level, mslp and precipitation names
MIXED = (("t_grid", 7, "min"), ("z_plev", 1, "quantile", 0.5), ("precnv", 0, "prob_above", 0.0), ("t_grid", 7, "max"),
         ("mslp", 0, "quantile", 0.25), ("z_plev", 1, "min"), ("u_grid", 0, "quantile", 0.9), ("precnv", 0, "max"),
         ("t_grid", 7, "quantile", 0.5))


def test_an_entry_is_a_function_of_its_own_plane_and_parameters(spectral, bc):
    """qtape_compute() under MIXED and, on the same state, under the same entries with equal planes adjacent: entry for entry the
    same bits at every point.  Holds the table of distinct planes (csrc/entry_front.hpp) to the order of the caller's list; the
    mask has two runs."""
    planes = [e[:2] for e in MIXED]
    order = sorted(range(len(MIXED)), key=lambda k: planes.index(planes[k]))
    assert order != list(range(len(MIXED)))
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, 4)
    try:
        model.set_bc(bc)
        perturb(model)
        model.plev_configure([850.0, 500.0])
        model.run(3)
        got = []
        for entries in (MIXED, [MIXED[k] for k in order]):
            model.qtape_configure(entries, (1, 0, 1, 1), EVERY, capacity=2, in_loop=False)
            got.append(model.qtape_compute().cpu().numpy())  # [E][48][96]
        assert got[0].shape == (len(MIXED), 48, 96) and np.isfinite(got[0]).all()
        assert np.array_equal(bits(got[0][order]), bits(got[1])), [k for k in range(len(MIXED)) if (got[0][order[k]] != got[1][k]).any()]
        assert (got[0][0] < got[0][8]).any() and (got[0][8] < got[0][3]).any() and (got[0][5] <= got[0][1]).all()  # (min, median, max)
    finally:
        model.close()
