"""GPU tier: the verification tape (spd_model_verif_*, csrc/verif.hip) against its definition restated in numpy
(tests/verif_reference.py, tests/projtape_reference.py; include/pyspeedy_amd.h).  Scores and histograms are
compared as bit patterns with the arbiter applied to the fp64 tape of a twin model sampled at the same steps.

Shapes: 5 members, truth 2, the other four masked (r = 4), and the same with r = 3; 8 members in 2 member groups and 2 rounds,
truth 6 (the last round, the second group), member 3 unused, r = 6; 66 members, r = 64, one verif_apply only.

Seven entries: t_grid at the lowest level under the global mean and under a box across the date line, u_grid level 0 under a
seeded N(0, 1) map, ps_grid, mslp under the box, z_plev at 500 hPa, precnv under the global mean (its dry points are real ties).

  1  every = 3 over calls of 5, 1, 7 and 12 steps from step 30: in-loop (a ring of 5 that wraps), the host loop run(k);
     verif_apply() (a ring of 16), checked calls; each row is the arbiter's on the twin's tape; verif_compute()
  2  isolation: every registry variable is bitwise that of a model without any recorder, a projection tape beside it holds the
     bits it holds alone
  3  66 members, one verif_apply
  4  beside in-loop assimilation (tests/test_assim_gpu.py's 8-member shape and entries): phase 0 the arbiter on the state before
     the analysis, phase 1 on the state after it, `analysis` 0 at the skipped event; states and the assimilation's ring are those
     of the run without verification
  5  refusals with a model: the truth inside the mask, a member index >= M, pressure-level names without levels, plev_configure
     while such an entry is configured, reads after a failed range check
"""
import ctypes as C

import numpy as np
import pytest

import verif_reference as ref
from test_breed_gpu import bc, bits, differing, perturb, registry  # noqa: F401

pytestmark = pytest.mark.gpu

START, EVERY, CALLS = 30, 3, (5, 1, 7, 12)  # (the first convective rain falls around step 24)
EVENTS = [s for s in range(START + 1, START + sum(CALLS) + 1) if s % EVERY == 0]  # 33, 36, ..., 54
SHAPES = {"5_members_r4": (5, (), (1, 1, 0, 1, 1), 2),
          "5_members_r3": (5, (), (1, 1, 0, 1, 0), 2),
          "8_members_2_groups_2_rounds": (8, (("member_groups", 2), ("block_members", 2)), (1, 1, 1, 0, 1, 1, 0, 1), 6)}
# patterns: 0 the global mean, 1 a box across the date line, 2 N(0, 1)
ENTRIES = (("t_grid", 7, 0), ("t_grid", 7, 1), ("u_grid", 0, 2), ("ps_grid", 0, 0), ("mslp", 0, 1), ("z_plev", 0, 0), ("precnv", 0, 0))
PRECNV = 6
TAPED = ("t_grid", "u_grid", "ps_grid", "mslp", "z_plev", "precnv")
PROJ_EVERY = 2


@pytest.fixture(scope="module")
def maps():
    import pyspeedy_amd
    pw = pyspeedy_amd.projection_weights()
    w = np.stack([pw.global_mean(), pw.box(150.0, -150.0, -40.0, 25.0), np.random.default_rng(2026).normal(0.0, 1.0, (48, 96))])
    assert (w[0] > 0).all() and 0 < np.count_nonzero(w[1]) < 4608 and w[2].all()
    return w


def fresh(spectral, bc, members, options=()):
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, members)
    model.set_bc(bc)
    for name, value in options:
        model.set_option(name, value)
    perturb(model)
    model.plev_configure([500.0])
    model.run(START)
    return model


def tape_planes(model, t):
    """{(name, level): [M][48][96]} of sample t of the model's fp64 tape, for the planes the entries name"""
    out = {}
    for name, level, _ in ENTRIES:
        if (name, level) not in out:
            x = model.tape(name, t0=t, nt=1)[:, 0].cpu().numpy()
            assert x.dtype == np.float64
            out[(name, level)] = x[:, level] if x.ndim == 4 else x
    return out


def ring_of(model):
    got = model.verif()
    return dict(scores=np.stack([got[k].cpu().numpy() for k in ref.NAMES], axis=-1), hist=model.verif_hist().cpu().numpy(),
                analysis=got["analysis"].cpu().numpy(), rmse=got["rmse"].cpu().numpy(), spread=got["spread"].cpu().numpy(),
                steps=model.verif_steps().tolist(), times=model.verif_times())


def same_rows(ring, first, scores, hists, r):
    """the ring's rows from event `first` on are the arbiter's in phase 0 and blank in phase 1"""
    n = len(ring["steps"])
    assert ring["scores"].shape == (n, 2, len(ENTRIES), 4) and ring["hist"].shape == (n, 2, len(ENTRIES), r + 2)
    for t in range(n):
        want, want_hist = scores[first + t], hists[first + t][:, :r + 2]
        assert np.array_equal(bits(ring["scores"][t, 0]), bits(want)), (t, int((bits(ring["scores"][t, 0]) != bits(want)).sum()))
        assert np.array_equal(ring["hist"][t, 0], want_hist), (t, ring["hist"][t, 0], want_hist)
    assert np.isnan(ring["scores"][:, 1]).all() and (ring["hist"][:, 1] == -1).all() and not ring["analysis"].any()
    for name, k in (("rmse", 1), ("spread", 2)):  # (the square root of a sum under a map of both signs may be NaN)
        square = ring["scores"][:, 0, :, k]
        ok = square >= 0
        assert np.array_equal(bits(ring[name][:, 0][ok]), bits(np.sqrt(square[ok]))) and np.isnan(ring[name][:, 0][~ok]).all(), name


class Plans:
    """The runs of one ensemble shape from step 30, each on a model of its own."""

    def __init__(self, spectral, bc, maps, members, options, mask, truth):
        self.members, self.mask, self.truth, self.models = members, mask, truth, []
        self.masked = [i for i in range(members) if mask[i]]

        def start():
            model = fresh(spectral, bc, members, options)
            self.models.append(model)
            return model

        # the twin: an fp64 tape and a projection tape, no verification
        twin = start()
        twin.tape_configure(TAPED, EVERY, len(EVENTS), dtype="float64")
        twin.projtape_configure(maps, ENTRIES, PROJ_EVERY, 16)
        for k in CALLS:
            twin.run(k)
        assert twin.tape_steps().tolist() == EVENTS
        rows = [ref.event(tape_planes(twin, t), truth, self.masked, ENTRIES, maps) for t in range(len(EVENTS))]
        self.scores, self.hists = [r[0] for r in rows], [r[1] for r in rows]
        self.proj_twin, self.times_twin = twin.projtape().cpu().numpy(), twin.tape_times()
        # in the loop, beside a projection tape; the ring wraps
        a = start()
        a.verif_configure(maps, ENTRIES, mask, truth, EVERY, capacity=5)
        a.projtape_configure(maps, ENTRIES, PROJ_EVERY, 16)
        self.info0 = a.verif_info()
        for k in CALLS:
            a.run(k)
        self.a, self.ring_a, self.info_a, self.proj_a = registry(a), ring_of(a), a.verif_info(), a.projtape().cpu().numpy()
        never = start()
        for k in CALLS:
            never.run(k)
        self.never = registry(never)
        # the host loop; verif_compute() in front of every verif_apply()
        b, self.computed = start(), []
        b.verif_configure(maps, ENTRIES, mask, truth, EVERY, capacity=16, in_loop=False)
        for k in CALLS:
            left = k
            while left:
                n = min(EVERY - b.current_step % EVERY, left)
                b.run(n)
                left -= n
                if b.current_step % EVERY == 0:
                    got = b.verif_compute()
                    self.computed.append((np.stack([got[name].cpu().numpy() for name in ref.NAMES], axis=-1), got["hist"].cpu().numpy()))
                    b.verif_apply()
        self.b, self.ring_b, self.info_b = registry(b), ring_of(b), b.verif_info()
        checked = start()
        checked.verif_configure(maps, ENTRIES, mask, truth, EVERY, capacity=16)
        self.codes = [checked.run_checked(k)[0] for k in CALLS]
        self.checked, self.ring_checked = registry(checked), ring_of(checked)
        # in_loop = False and no verif_apply: nothing is recorded
        idle = start()
        idle.verif_configure(maps, ENTRIES, mask, truth, EVERY, capacity=4, in_loop=False)
        idle.run(CALLS[0] + CALLS[1])
        self.info_idle = idle.verif_info()
        idle.verif_off()
        self.info_off = idle.verif_info()

    def close(self):
        for model in self.models:
            model.close()


@pytest.fixture(scope="module", params=list(SHAPES))
def plans(request, spectral, bc, maps):
    p = Plans(spectral, bc, maps, *SHAPES[request.param])
    yield p
    p.close()


# ---- 1: the schedule and the arithmetic ----------------------------------------------------------------------------------------
def test_in_loop_rows_are_the_arbiters_on_the_twins_tape(plans):
    r = len(plans.masked)
    assert plans.info0 == dict(members=r, truth=plans.truth, entries=len(ENTRIES), every=EVERY, capacity=5, taken=0, held=0, in_loop=True,
                               applied=0)
    assert (plans.info_a["taken"], plans.info_a["held"], plans.info_a["applied"]) == (len(EVENTS), 5, len(EVENTS))
    assert plans.ring_a["steps"] == EVENTS[-5:] and plans.ring_a["times"] == plans.times_twin[-5:]  # (the ring wrapped)
    same_rows(plans.ring_a, len(EVENTS) - 5, plans.scores, plans.hists, r)
    if plans.members == 8:
        assert (plans.models[0].config()["chunks"], plans.models[0].config()["rounds"]) == (2, 2)


def test_the_arbiters_series_vary_and_the_ties_are_the_dry_points(plans, maps):
    r = len(plans.masked)
    scores, hists = np.stack(plans.scores), np.stack(plans.hists)  # [T][E][4], [T][E][66]
    assert np.isfinite(scores).all()
    for e in range(len(ENTRIES)):
        for k in range(4):
            assert len(set(bits(scores[:, e, k]).tolist())) == len(EVENTS), (e, k)  # no two events alike
    for k in range(4):
        assert len(set(bits(scores[-1, :, k]).tolist())) == len(ENTRIES), k  # no two entries alike
    positive = [e for e, (_, _, pattern) in enumerate(ENTRIES) if pattern != 2]  # (under a map without a negative weight)
    assert (scores[:, positive, 1:] > 0).all()  # mse, variance and crps of members that differ
    ties = hists[:, :, r + 1]
    assert (ties[:, :PRECNV] == 0).all() and (ties[:, PRECNV] > 0).all(), ties
    assert (hists[:, PRECNV, :r + 1].sum(axis=1) > 0).all()  # (it rains somewhere: not every point is a tie)
    assert not hists[:, :, r + 2:].any()
    # every point under a weight is counted once; the device's rows say the same
    for e, (_, _, pattern) in enumerate(ENTRIES):
        assert (hists[:, e].sum(axis=1) == np.count_nonzero(maps[pattern])).all(), e
    got = plans.ring_a["hist"][:, 0]
    assert (got[:, :PRECNV, r + 1] == 0).all() and (got[:, PRECNV, r + 1] > 0).all()


def test_in_loop_is_the_host_loop_and_the_checked_call(plans):
    r = len(plans.masked)
    assert plans.ring_b["steps"] == plans.ring_checked["steps"] == EVENTS  # (these rings do not wrap)
    same_rows(plans.ring_b, 0, plans.scores, plans.hists, r)
    same_rows(plans.ring_checked, 0, plans.scores, plans.hists, r)
    assert plans.ring_b["times"] == plans.ring_checked["times"] == plans.times_twin
    for t, (scores, hist) in enumerate(plans.computed):  # verif_compute() in front of each verif_apply()
        assert np.array_equal(bits(scores), bits(plans.scores[t])) and np.array_equal(hist, plans.hists[t][:, :r + 2]), t
    assert len(plans.computed) == len(EVENTS) and plans.info_b["taken"] == len(EVENTS) and not plans.info_b["in_loop"]
    assert all((codes == -1).all() for codes in plans.codes)
    assert plans.info_idle["taken"] == 0 and plans.info_idle["members"] == r
    assert plans.info_off == dict(members=0, truth=-1, entries=0, every=0, capacity=0, taken=0, held=0, in_loop=False, applied=0)


# ---- 2: isolation -----------------------------------------------------------------------------------------------------------
def test_the_recorder_changes_no_state_bit_and_no_other_ring(plans):
    assert differing(plans.a, plans.never) == []        # the extra cuts and the events move nothing
    assert differing(plans.b, plans.never) == [] and differing(plans.checked, plans.never) == []
    assert plans.proj_a.shape == plans.proj_twin.shape == (plans.members, (START + sum(CALLS)) // PROJ_EVERY - START // PROJ_EVERY, len(ENTRIES))
    assert np.array_equal(bits(plans.proj_a), bits(plans.proj_twin))


# ---- 3: the largest ensemble ------------------------------------------------------------------------------------------------
def test_sixty_four_members_in_one_apply(spectral, bc, maps):
    members, truth = 66, 40
    mask = np.ones(members, dtype=np.int32)
    mask[[0, truth]] = 0
    masked = np.flatnonzero(mask).tolist()
    twin, model = fresh(spectral, bc, members), fresh(spectral, bc, members)
    try:
        twin.tape_configure(TAPED, 3, 1, dtype="float64")
        twin.run(3)
        assert twin.tape_steps().tolist() == [START + 3]
        scores, hists = ref.event(tape_planes(twin, 0), truth, masked, ENTRIES, maps)
        model.verif_configure(maps, ENTRIES, mask, truth, 5, capacity=2, in_loop=False)
        assert model.verif_info()["members"] == 64
        model.run(3)
        model.verif_apply()
        ring = ring_of(model)
        assert ring["steps"] == [START + 3]
        same_rows(ring, 0, [scores], [hists], 64)
        assert (hists[:PRECNV, 65] == 0).all() and hists[PRECNV, 65] > 0 and (hists[:, :66].sum(axis=1) > 0).all()
        assert np.count_nonzero(hists[0, :65]) > 32  # (the ranks spread over the histogram)
    finally:
        twin.close()
        model.close()


# ---- 4: beside the in-loop assimilation -----------------------------------------------------------------------------------------
def snapshot(model, views):
    """what an fp64 tape would hold of the state as it stands (tests/test_tape_gpu.py holds the tape to exactly this)"""
    model.spectral2grid()
    pl = model.plev(["z_plev", "mslp"])
    out = {}
    for name, level, _ in ENTRIES:
        x = pl[name] if name in pl else views[name].double()
        out[(name, level)] = (x[:, level] if x.dim() == 4 else x).cpu().numpy().copy()
    return out


def test_beside_in_loop_assimilation_both_phases_are_the_arbiters(spectral, bc, maps):
    import pyspeedy_amd
    import test_assim_gpu as ta
    members, options, mask = ta.SHAPES["8_members_2_groups_2_rounds"]
    truth, masked = 2, [i for i in range(members) if mask[i]]
    assert mask[truth] == 0
    amaps = np.stack([pyspeedy_amd.projection_weights().point(*ta.STATION), maps[1], maps[2], maps[0], np.zeros((48, 96))])
    models = []

    def start(in_loop):
        model = ta.fresh(spectral, bc, members, options)
        models.append(model)
        views = {n: model.device_view(n) for n in ("t_grid", "u_grid", "ps_grid", "precnv")}
        model.assim_configure(amaps, ta.ENTRIES, mask, ta.EVERY, capacity=8, inflation=1.05, in_loop=in_loop)
        return model, views

    try:
        # the host loop without verification: observations from its own priors, the planes before and after every event
        host, views = start(False)
        table, before, after = [], {}, {}

        while host.current_step < ta.START + ta.STEPS:
            host.run(min(ta.EVERY - host.current_step % ta.EVERY, ta.START + ta.STEPS - host.current_step))
            if host.current_step % ta.EVERY == 0:
                before[host.current_step] = snapshot(host, views)
            if host.current_step in ta.ROWS:
                table.append(ta.observations(host.assim_compute().cpu().numpy()))
                host.assim_observations(ta.ROWS[:len(table)], np.stack([t[0] for t in table]), np.stack([t[1] for t in table]))
                host.assim_apply()
                after[host.current_step] = snapshot(host, views)
        events = sorted(before)
        assert events == [32, 36, 40] and sorted(after) == list(ta.ROWS)
        plain, _ = start(True)
        both, _ = start(True)
        both.verif_configure(maps, ENTRIES, mask, truth, ta.EVERY, capacity=8)
        for model in (plain, both):
            model.assim_observations(ta.ROWS, np.stack([t[0] for t in table]), np.stack([t[1] for t in table]))
            model.run(ta.STEPS)
        ring = ring_of(both)
        r = len(masked)
        assert ring["steps"] == events and ring["analysis"].tolist() == [1, 0, 1]
        for t, step in enumerate(events):
            for phase, planes in ((0, before[step]), (1, after.get(step))):
                got, got_hist = ring["scores"][t, phase], ring["hist"][t, phase]
                if planes is None:  # the skipped event: no analysis, no second phase
                    assert np.isnan(got).all() and (got_hist == -1).all()
                    continue
                want, want_hist = ref.event(planes, truth, masked, ENTRIES, maps)
                assert np.array_equal(bits(got), bits(want)), (step, phase, int((bits(got) != bits(want)).sum()))
                assert np.array_equal(got_hist, want_hist[:, :r + 2]), (step, phase)
        # the analysis moved the scores of the fields it corrects, and left precnv (an output of the physics) alone
        assert not np.array_equal(bits(ring["scores"][0, 0, :PRECNV]), bits(ring["scores"][0, 1, :PRECNV]))
        assert np.array_equal(bits(ring["scores"][0, 0, PRECNV]), bits(ring["scores"][0, 1, PRECNV]))
        # states and the assimilation's ring are those of the run without verification, and of the host loop
        reg = registry(both)
        assert differing(reg, registry(plain)) == []
        # (the host loop's snapshots filled the registry's exported grid arrays, which a stepped model never writes)
        assert {n for n, _ in differing(reg, registry(host))} <= {"u_grid", "v_grid", "t_grid", "q_grid", "phi_grid", "ps_grid"}
        assert ta.same_ring(ta.ring_of(both), ta.ring_of(plain)) and ta.same_ring(ta.ring_of(both), ta.ring_of(host))
        assert both.assim_info() == plain.assim_info() and both.assim_info()["skipped"] == 1
    finally:
        for model in models:
            model.close()


# ---- 5: refusals that need a model ----------------------------------------------------------------------------------------------
def test_refusals_and_lifecycle(spectral, bc, maps):
    from pyspeedy_amd import SpeedyHipError
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, 4)
    try:
        model.set_bc(bc)
        perturb(model)
        with pytest.raises(SpeedyHipError, match="'mslp' needs target levels"):
            model.verif_configure(maps, ENTRIES, (1, 1, 1, 0), 3, EVERY)
        model.plev_configure([500.0])
        with pytest.raises(SpeedyHipError, match="the truth member 1 is masked in"):
            model.verif_configure(maps, ENTRIES, (1, 1, 1, 0), 1, EVERY)
        with pytest.raises(SpeedyHipError, match=r"the truth member 4 is out of range \(0 ... 3\)"):
            model.verif_configure(maps, ENTRIES, (1, 1, 1, 0), 4, EVERY)
        with pytest.raises(SpeedyHipError, match="1 members are masked in"):
            model.verif_configure(maps, ENTRIES, (1, 0, 0, 0), 3, EVERY)
        with pytest.raises(SpeedyHipError, match="no verification tape configured"):
            model.verif_apply()
        assert model.verif_info()["members"] == 0 and model.verif_entries == ()
        model.verif_configure(maps, ENTRIES, (1, 1, 1, 0), 3, EVERY, capacity=4)
        assert model.verif_entries == ENTRIES
        with pytest.raises(SpeedyHipError, match="the verification tape holds a pressure-level variable"):
            model.plev_configure([850.0])
        model.run(EVERY)
        assert model.verif_steps().tolist() == [EVERY]
        model.verif_reset()
        assert model.verif_info()["taken"] == 0 and model.verif()["bias"].shape == (0, 2, len(ENTRIES))
        with pytest.raises(SpeedyHipError, match="event range out of bounds"):
            model.verif(0, 1)
        # a checked call in flight
        stream = model._stream()
        assert model._lib.spd_model_step_checked_begin(model._m, EVERY, stream) == 0
        for call in (model.verif, model.verif_hist, model.verif_apply, model.verif_compute, model.verif_reset, model.verif_off,
                     lambda: model.verif_configure(maps, ENTRIES, (1, 1, 1, 0), 3, EVERY)):
            with pytest.raises(SpeedyHipError, match="in flight"):
                call()
        failed = np.zeros(4, dtype=np.int32)
        assert model._lib.spd_model_step_checked_end(model._m, failed.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
        assert failed.tolist() == [-1] * 4 and model.verif_steps().tolist() == [2 * EVERY]
        # a member out of range: global-mean temperature of 500 K (diagnostics.f90:57-66), as tests/test_tape_gpu.py
        t = model.get("t", 1)
        t[0, 0, :, :] = 500.0 * np.sqrt(2.0)
        model.set("t", t, member=1)
        failed, _ = model.run_checked(EVERY)
        assert failed.tolist() == [-1, 0, -1, -1]
        with pytest.raises(SpeedyHipError, match="the verification tape is invalid until spd_model_verif_reset: member 1 failed the range check"):
            model.verif()
        with pytest.raises(SpeedyHipError, match="the verification tape is invalid"):
            model.verif_hist()
        assert model.verif_info()["taken"] == 2  # (the count is still told)
        model.verif_reset()
        assert model.verif()["analysis"].shape == (0,)
        # spd_model_init: an empty ring, the configuration stays
        model.init((1982, 1, 1, 0, 0))
        model.run(EVERY)
        assert model.verif_info()["taken"] == 1
        model.init((1982, 1, 1, 0, 0))
        assert model.verif_info()["taken"] == 0 and model.verif_info()["members"] == 3
    finally:
        model.close()


# an interleaved list that comes back to planes it has left (t_grid 7, z_plev 1 and precnv, not adjacent) and mixes sigma-level,
# pressure-level, mslp and precipitation names
MIXED = (("t_grid", 7, 0), ("z_plev", 1, 1), ("precnv", 0, 0), ("t_grid", 7, 2), ("mslp", 0, 1), ("z_plev", 1, 0), ("u_grid", 0, 2),
         ("precnv", 0, 1), ("t_grid", 7, 1))


def test_an_entry_is_a_function_of_its_own_plane_and_pattern(spectral, bc, maps):
    """verif_compute() under MIXED and, on the same state, under the same entries with equal planes adjacent: entry for entry the
    same bits in every score and the same histogram.  Holds the table of distinct planes (csrc/entry_front.hpp) to the order of the
    caller's list; the truth, member 2, lies between the two runs of the mask."""
    planes = [e[:2] for e in MIXED]
    order = sorted(range(len(MIXED)), key=lambda k: planes.index(planes[k]))
    assert order != list(range(len(MIXED)))
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, 5)
    try:
        model.set_bc(bc)
        perturb(model)
        model.plev_configure([850.0, 500.0])
        model.run(3)
        got = []
        for entries in (MIXED, [MIXED[k] for k in order]):
            model.verif_configure(maps, entries, (1, 1, 0, 1, 1), 2, EVERY, capacity=2, in_loop=False)
            got.append({k: v.cpu().numpy() for k, v in model.verif_compute().items()})
        for name in ref.NAMES:
            assert got[0][name].shape == (len(MIXED),)
            assert np.array_equal(bits(got[0][name][order]), bits(got[1][name])), (name, got[0][name][order], got[1][name])
        assert got[0]["hist"].shape == (len(MIXED), 6) and np.array_equal(got[0]["hist"][order], got[1]["hist"])
        dry = [k for k, e in enumerate(MIXED) if e[0] != "precnv"]
        assert len(np.unique(got[0]["mse"][dry])) == len(dry) and (got[0]["hist"].sum(axis=1) > 0).all()
    finally:
        model.close()
