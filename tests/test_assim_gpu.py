"""GPU tier: the assimilation (spd_model_assim_*, csrc/assim.hip) against its definition restated in numpy
(tests/assim_reference.py, tests/projtape_reference.py; include/pyspeedy_amd.h).  States, weights and rings are
compared as bit patterns.

Shapes: 4 members, mask [0, 1, 1, 1]; 8 members in 2 member groups and 2 rounds, mask [1, 1, 0, 1, 1, 1, 0, 1] (masked members in
different groups and rounds); 20 members, mask [0] + [1] * 19, one assim_apply only (partial blocks of eight in the transform).

Seven entries: t_grid at the lowest level under a station stencil and under a box across the date line, u_grid level 0 under a
seeded N(0, 1) map, the global mean of ps_grid, an mslp box, an entry whose observation is NaN, an entry under an all-zero map.

  1  assim_compute() is the projection-tape ring of a twin model sampled at that step; it writes nothing
  2  one assim_apply(): W and the ring slot are the arbiter's on the device's own Y, both time levels of all five variables are
     the arbiter's transform, and nothing else moves
  3  assim_transform(): the identity, a permutation, a seeded dense matrix
  4  a single linear entry: the analytic posterior mean and variance
  5  in-loop run(12), 12 x run(1), the host loop, an unconfigured model moved by the arbiter through get / set, a checked call;
     the quiet rim
  6  assim_off(), in-loop breeding beside in-loop assimilation, nudging beside assimilation
"""
import numpy as np
import pytest

import assim_reference as ref
from test_breed_gpu import EVERY, SPEC, START, STEPS, bc, bits, differing, member_state, perturb, registry  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = {"4_members": (4, (), (0, 1, 1, 1)),
          "8_members_2_groups_2_rounds": (8, (("member_groups", 2), ("block_members", 2)), (1, 1, 0, 1, 1, 1, 0, 1)),
          "20_members_apply_only": (20, (), (0,) + (1,) * 19)}
STATION = (39.0, -30.0)
# patterns: 0 the station, 1 a box across the date line, 2 N(0, 1), 3 the global mean, 4 all zero
ENTRIES = (("t_grid", 7, 0), ("t_grid", 7, 1), ("u_grid", 0, 2), ("ps_grid", 0, 3), ("mslp", 0, 1), ("v_grid", 4, 3), ("q_grid", 5, 4))
MISSING, ZERO_MAP = 5, 6
USED = [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
ROWS = (32, 40)  # the stamps of the in-loop case: the event of step 36 finds no row


@pytest.fixture(scope="module")
def maps():
    import pyspeedy_amd
    pw = pyspeedy_amd.projection_weights()
    w = np.stack([pw.point(*STATION), pw.box(150.0, -150.0, -40.0, 25.0), np.random.default_rng(2025).normal(0.0, 1.0, (48, 96)),
                  pw.global_mean(), np.zeros((48, 96))])
    assert np.count_nonzero(w[0]) == 4 and (w[0] >= 0).all() and abs(w[0].sum() - 1.0) < 1e-12 and not w[4].any()
    return w


def fresh(spectral, bc, members, options=(), steps=START):
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, members)
    model.set_bc(bc)
    for name, value in options:
        model.set_option(name, value)
    perturb(model)
    model.plev_configure([500.0])  # (mslp is the pressure-level kernel's)
    if steps:
        model.run(steps)
    return model


def observations(Y):
    """From an observation-space ensemble [E][r]: observations 0.7 prior standard deviations off the prior mean, to alternating
    sides, with error variances equal to the prior variances (1.0 where the prior has none); the entry MISSING is NaN."""
    mean, var = Y.mean(axis=1), Y.var(axis=1, ddof=1)
    yo = mean + 0.7 * np.sqrt(var) * np.where(np.arange(len(mean)) % 2 == 0, 1.0, -1.0)
    yo[MISSING] = np.nan
    return yo, np.where(var > 0.0, var, 1.0)


def ring_of(model):
    got = model.assim()
    return dict(stats=np.stack([got[k].cpu().numpy() for k in ("mean", "variance", "innovation", "used")], axis=-1),
                steps=model.assim_steps().tolist(), times=model.assim_times())


def same_ring(a, b):
    return np.array_equal(bits(a["stats"]), bits(b["stats"])) and a["steps"] == b["steps"] and a["times"] == b["times"]


def arbiter_event(reg, masked, W):
    """the registry the transform with W makes of `reg`"""
    expected = {n: list(v) for n, v in reg.items()}
    moved = ref.transform([member_state(reg, i) for i in masked], W)
    for j, i in enumerate(masked):
        for n in SPEC:
            expected[n][i] = moved[j][n]
    return expected


# ---- 1: the observation operator ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["4_members", "8_members_2_groups_2_rounds"])
def test_compute_is_the_projection_tape_of_a_twin(spectral, bc, maps, shape):
    members, options, mask = SHAPES[shape]
    masked = [i for i in range(members) if mask[i]]
    twin = fresh(spectral, bc, members, options, steps=0)
    model = fresh(spectral, bc, members, options)
    try:
        twin.projtape_configure(maps, ENTRIES, START, 1)
        twin.run(START)
        assert twin.projtape_steps().tolist() == [START]
        want = twin.projtape().cpu().numpy()  # [members][1][E]
        model.assim_configure(maps, ENTRIES, mask, EVERY, capacity=2, in_loop=False)
        before = registry(model)
        got = model.assim_compute().cpu().numpy()
        assert got.shape == (len(ENTRIES), len(masked))
        assert np.array_equal(bits(got), bits(want[masked, 0, :].T)), int((bits(got) != bits(want[masked, 0, :].T)).sum())
        assert differing(registry(model), before) == [] and model.assim_info()["taken"] == 0  # (it writes nothing)
        assert not got[ZERO_MAP].any() and got[:ZERO_MAP].all() and (got[:ZERO_MAP].var(axis=1) > 0).all()
    finally:
        twin.close()
        model.close()


# ---- 2: one assim_apply ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_apply_is_the_definition(spectral, bc, maps, shape):
    from pyspeedy_amd import SpeedyHipError
    members, options, mask = SHAPES[shape]
    masked = [i for i in range(members) if mask[i]]
    model = fresh(spectral, bc, members, options)
    try:
        if members == 8:
            assert (model.config()["chunks"], model.config()["rounds"]) == (2, 2)
        model.assim_configure(maps, ENTRIES, mask, EVERY, capacity=2, inflation=1.05, in_loop=False)
        assert model.assim_info() == dict(members=len(masked), entries=len(ENTRIES), every=EVERY, capacity=2, taken=0, held=0, skipped=0,
                                          in_loop=False, applied=0)
        with pytest.raises(SpeedyHipError, match="no row of observations is stamped with the current step"):
            model.assim_apply()
        with pytest.raises(SpeedyHipError, match="no event has been executed"):
            model.assim_weights()
        Y = model.assim_compute().cpu().numpy()
        yo, R = observations(Y)
        model.assim_observations([START - 1, START], np.stack([yo + 1.0, yo]), np.stack([R, R]))
        before = registry(model)
        model.assim_apply()
        after, ring, got = registry(model), ring_of(model), model.assim_weights()
        info = model.assim_info()
        assert (info["taken"], info["applied"], info["skipped"]) == (1, 1, 0) and ring["steps"] == [START]
        # the device's own Y is what assim_compute showed; W and the ring slot are the arbiter's on it
        Yd, Wd = got["Y"].cpu().numpy(), got["W"].cpu().numpy()
        assert np.array_equal(bits(Yd), bits(Y)) and Wd.shape == (len(masked), len(masked))
        W, stats = ref.weights(Yd, yo, R, 1.05)
        assert np.array_equal(bits(Wd), bits(W)), int((bits(Wd) != bits(W)).sum())
        assert np.array_equal(bits(ring["stats"][0]), bits(stats)), int((bits(ring["stats"][0]) != bits(stats)).sum())
        assert stats[:, 3].tolist() == USED and stats[MISSING, 2] == 0.0 and stats[ZERO_MAP, 1] == 0.0
        # the states
        expected = arbiter_event(before, masked, W)
        for i in masked:
            for n in SPEC:
                assert not np.array_equal(bits(expected[n][i]), bits(before[n][i])), (n, i)  # (the case moves the state)
                assert np.array_equal(bits(after[n][i]), bits(expected[n][i])), (n, i, int((bits(after[n][i]) != bits(expected[n][i])).sum()))
                assert np.array_equal(bits(after[n][i][~ref.INSIDE]), bits(before[n][i][~ref.INSIDE])), (n, i)
        assert differing(after, expected) == []  # (the members outside the mask and every other registry variable: unchanged)
    finally:
        model.close()


# ---- 3: the caller's matrix -----------------------------------------------------------------------------------------------------
def test_transform_with_the_callers_matrix(spectral, bc):
    from pyspeedy_amd import SpeedyHipError
    model = fresh(spectral, bc, 4, steps=3)
    try:
        start = registry(model)
        model.assim_transform([0, 1, 2, 3], np.eye(4))
        assert differing(registry(model), start) == []  # the identity leaves the bits
        perm = [2, 0, 1]  # member [1, 2, 3][j] takes the state of member [1, 2, 3][perm[j]]
        P = np.zeros((3, 3))
        for j, i in enumerate(perm):
            P[i, j] = 1.0
        model.assim_transform([1, 2, 3], P)
        after = registry(model)
        for n in SPEC:
            assert np.array_equal(bits(after[n][0]), bits(start[n][0]))
            for j, i in enumerate(perm):
                assert np.array_equal(bits(after[n][1 + j]), bits(start[n][1 + i])), (n, j)
                assert not np.array_equal(bits(after[n][1 + j]), bits(start[n][1 + j])), (n, j)
        W = np.random.default_rng(17).standard_normal((3, 3))
        model.assim_transform([3, 0, 2], W)  # (any order of distinct members)
        expected = {n: list(v) for n, v in after.items()}
        moved = ref.transform([member_state(after, i) for i in (3, 0, 2)], W)
        for j, i in enumerate((3, 0, 2)):
            for n in SPEC:
                expected[n][i] = moved[j][n]
        final = registry(model)
        assert differing(final, expected) == []
        assert sorted({i for n, i in differing(final, after)}) == [0, 2, 3]
        with pytest.raises(SpeedyHipError, match=r"member 4 is out of range \(0 ... 3\)"):
            model.assim_transform([0, 4], np.eye(2))
        assert model.assim_info()["members"] == 0  # (no assimilation was ever configured)
    finally:
        model.close()


# ---- 4: the analytic posterior ------------------------------------------------------------------------------------------------
def test_a_single_linear_entry_shows_the_analytic_posterior(spectral, bc, maps):
    """One used entry, t_grid at the lowest level under the station stencil (linear in the spectral state), rho = 1, 19 members.
    With ybar, s, v of the ring and R: the posterior mean is ybar + s / (s + R) v and the posterior variance s R / (s + R).
    assim_compute() after the event goes through the transform of 33 planes, the export transforms and the projection again, so
    the comparison is held to B = 64 x 4608 x 2^-53 x sum |w| |x| on the mean and 2 sqrt(s) B on the variance; the stencil's
    weights are not negative and sum to 1 and T > 0, so sum |w| |x| is the entry's own value (its largest over the members).
    The ensemble's sqrt(s) must exceed 1e4 B for the case to say anything."""
    members, options, mask = SHAPES["20_members_apply_only"]
    model = fresh(spectral, bc, members, options)
    try:
        model.assim_configure(maps[:1], ENTRIES[:1], mask, EVERY, capacity=1, in_loop=False)
        Y = model.assim_compute().cpu().numpy()
        B = 64 * 4608 * 2.0 ** -53 * float(np.abs(Y).max())
        s0 = float(Y.var(ddof=1))
        print("sqrt(s) = %.3e, B = %.3e" % (np.sqrt(s0), B))
        assert np.sqrt(s0) > 1e4 * B
        yo, R = float(Y.mean() + 1.5 * np.sqrt(s0)), 0.5 * s0
        model.assim_observations([START], [[yo]], [[R]])
        model.assim_apply()
        ybar, s, v, used = ring_of(model)["stats"][0, 0]
        assert used == 1.0
        Y2 = model.assim_compute().cpu().numpy()
        err_mean = abs(float(Y2.mean()) - (ybar + s / (s + R) * v))
        err_var = abs(float(Y2.var(ddof=1)) - s * R / (s + R))
        print("posterior mean off by %.3e (bound %.3e), variance off by %.3e (bound %.3e)" % (err_mean, B, err_var, 2 * np.sqrt(s) * B))
        assert err_mean <= B and err_var <= 2 * np.sqrt(s) * B, (err_mean, B, err_var, 2 * np.sqrt(s) * B)
        assert abs(float(Y2.mean()) - ybar) > 0.5 * np.sqrt(s)  # (the mean moved)
    finally:
        model.close()


# ---- 5, 6: the plans ------------------------------------------------------------------------------------------------------------
def host_loop(model, event):
    """run to the next multiple of EVERY and call event() at the stamped steps, until START + STEPS"""
    while model.current_step < START + STEPS:
        model.run(min(EVERY - model.current_step % EVERY, START + STEPS - model.current_step))
        if model.current_step in ROWS:
            event()


class Plans:
    """The runs of one ensemble shape from the same start (step 30), each on a model of its own."""

    def __init__(self, spectral, bc, maps, members, options, mask):
        self.members, self.mask, self.models = members, mask, []
        self.masked = [i for i in range(members) if mask[i]]

        def start():
            model = fresh(spectral, bc, members, options)
            self.models.append(model)
            return model

        def configured(in_loop=True):
            model = start()
            model.assim_configure(maps, ENTRIES, mask, EVERY, capacity=8, inflation=1.05, in_loop=in_loop)
            if self.table:
                model.assim_observations(ROWS, np.stack([t[0] for t in self.table]), np.stack([t[1] for t in self.table]))
            return model

        never = start()
        never.device_view("phi")  # (the fold pinned off, so that the rim looks in a small ensemble)
        never.run(STEPS)
        self.never, self.rim_never = registry(never), never.get_option("quiet_rim_members")
        # the host loop first: it makes the observations from its own priors, and keeps the device's Y and W of every event
        self.table, self.events = [], []
        b = configured(in_loop=False)

        def event():
            Y = b.assim_compute().cpu().numpy()
            self.table.append(observations(Y))
            b.assim_observations(ROWS[:len(self.table)], np.stack([t[0] for t in self.table]), np.stack([t[1] for t in self.table]))
            b.assim_apply()
            got = b.assim_weights()
            self.events.append((got["Y"].cpu().numpy(), got["W"].cpu().numpy()))

        host_loop(b, event)
        self.b, self.ring_b, self.info_b = registry(b), ring_of(b), b.assim_info()
        a = configured()
        self.fold_a = a.config()["fold_geo"]
        a.run(STEPS)
        self.a, self.ring_a, self.info_a, self.rim_a = registry(a), ring_of(a), a.assim_info(), a.get_option("quiet_rim_members")
        a1 = configured()
        for _ in range(STEPS):
            a1.run(1)
        self.a1, self.ring_a1, self.info_a1 = registry(a1), ring_of(a1), a1.assim_info()
        # an unconfigured model that the arbiter moves through get / set, on the device's own Y of the host loop's events
        c, self.rows_c = start(), []

        def arbiter():
            Y, _ = self.events[len(self.rows_c)]
            yo, R = self.table[len(self.rows_c)]
            W, stats = ref.weights(Y, yo, R, 1.05)
            self.rows_c.append((W, stats))
            reg = {n: [c.get(n, i) for i in range(members)] for n in SPEC}
            expected = arbiter_event(reg, self.masked, W)
            for i in self.masked:
                for n in SPEC:
                    c.set(n, expected[n][i], i)

        host_loop(c, arbiter)
        self.c = registry(c)
        checked = configured()
        self.codes, self.accepted = checked.run_checked(STEPS)
        self.checked, self.ring_checked, self.info_checked = registry(checked), ring_of(checked), checked.assim_info()
        gone = configured()
        gone.assim_off()
        self.fold_gone = gone.config()["fold_geo"]
        gone.run(STEPS)
        self.gone, self.info_gone = registry(gone), gone.assim_info()

    def close(self):
        for model in self.models:
            model.close()


@pytest.fixture(scope="module", params=["4_members", "8_members_2_groups_2_rounds"])
def plans(request, spectral, bc, maps):
    p = Plans(spectral, bc, maps, *SHAPES[request.param])
    yield p
    p.close()


def test_in_loop_assimilation_is_the_host_loop_and_the_arbiter(plans):
    assert (START + STEPS) % EVERY != 0 and START % EVERY != 0  # (the call neither starts nor ends at an event step)
    assert plans.ring_a["steps"] == list(ROWS)
    assert (plans.info_a["taken"], plans.info_a["applied"], plans.info_a["skipped"]) == (2, 2, 1)  # (step 36 has no row)
    assert (plans.info_a1["taken"], plans.info_a1["applied"], plans.info_a1["skipped"]) == (2, 2, 1)
    assert (plans.info_b["taken"], plans.info_b["applied"], plans.info_b["skipped"]) == (2, 2, 0)
    assert {i for n, i in differing(plans.a, plans.never)} == set(plans.masked)  # the case moves every masked member, and nobody else
    assert differing(plans.a1, plans.a) == []  # calls of one step
    assert differing(plans.b, plans.a) == []   # the host loop
    assert differing(plans.c, plans.a) == []   # the arbiter between the calls
    assert same_ring(plans.ring_a1, plans.ring_a) and same_ring(plans.ring_b, plans.ring_a)
    for k, (W, stats) in enumerate(plans.rows_c):
        assert np.array_equal(bits(plans.ring_a["stats"][k]), bits(stats)), k
        assert np.array_equal(bits(plans.events[k][1]), bits(W)), k
        assert stats[:, 3].tolist() == USED
    assert not plans.fold_a  # (no look-ahead geopotential while assimilation loops)


def test_a_checked_call_and_the_quiet_rim(plans):
    assert differing(plans.checked, plans.a) == [] and same_ring(plans.ring_checked, plans.ring_a)
    assert plans.info_checked["skipped"] == 1
    assert (plans.codes == -1).all(), plans.codes  # (no step of any member failed its range check)
    assert (plans.accepted[:, 0] == START + STEPS).all()
    print("quiet rim: %d with assimilation, %d in a plain run" % (plans.rim_a, plans.rim_never))
    assert plans.rim_a == plans.rim_never == plans.members


def test_off_means_off(plans):
    assert plans.info_gone == dict(members=0, entries=0, every=0, capacity=0, taken=0, held=0, skipped=0, in_loop=False, applied=0)
    assert differing(plans.gone, plans.never) == []
    assert plans.fold_gone  # (the look-ahead is back)


def test_breeding_and_assimilation_do_not_loop_together(spectral, bc, maps):
    from pyspeedy_amd import SpeedyHipError
    model = fresh(spectral, bc, 4, steps=3)
    try:
        model.breed_configure([-1, 0, 0, 0], 1e-3, EVERY)
        with pytest.raises(SpeedyHipError, match="in-loop assimilation cannot be configured while in-loop breeding"):
            model.assim_configure(maps, ENTRIES, (0, 1, 1, 1), EVERY)
        assert model.assim_info()["members"] == 0
        model.assim_configure(maps, ENTRIES, (0, 1, 1, 1), EVERY, in_loop=False)  # (one of them out of the loop: fine)
        model.breed_off()
        model.assim_configure(maps, ENTRIES, (0, 1, 1, 1), EVERY)
        with pytest.raises(SpeedyHipError, match="in-loop breeding cannot be configured while in-loop assimilation"):
            model.breed_configure([-1, 0, 0, 0], 1e-3, EVERY)
        assert model.breed_info()["bred"] == 0
        model.breed_configure([-1, 0, 0, 0], 1e-3, EVERY, in_loop=False)
    finally:
        model.close()


def test_nudging_in_the_loop_beside_assimilation_is_its_host_loop(spectral, bc, maps):
    from pyspeedy_amd import nudge_gains
    mask, got = (0, 1, 1, 1), []
    table = None
    for in_loop in (False, True):
        model = fresh(spectral, bc, 4)
        try:
            target = model.get("t", 0)[..., 0]
            model.nudge_configure({"t": nudge_gains(6.0)}, members=[0, 1, 1, 0], capacity=1)
            model.nudge_targets([START], {"t": target[None]})
            model.assim_configure(maps, ENTRIES, mask, EVERY, capacity=4, inflation=1.05, in_loop=in_loop)
            if in_loop:
                model.assim_observations(ROWS, np.stack([t[0] for t in table]), np.stack([t[1] for t in table]))
                model.run(STEPS)
            else:
                table = []

                def event():
                    table.append(observations(model.assim_compute().cpu().numpy()))
                    model.assim_observations(ROWS[:len(table)], np.stack([t[0] for t in table]), np.stack([t[1] for t in table]))
                    model.assim_apply()

                host_loop(model, event)
            got.append((registry(model), ring_of(model), model.nudge_info()["applied"]))
        finally:
            model.close()
    assert got[0][2] == got[1][2] == STEPS
    assert differing(got[1][0], got[0][0]) == [] and same_ring(got[1][1], got[0][1])
    assert got[0][1]["steps"] == list(ROWS)


# an interleaved list that comes back to planes it has left (t_grid 7 and z_plev 1, not adjacent) and mixes sigma-level,
# pressure-level and mslp names (precnv is refused here)
MIXED = (("t_grid", 7, 0), ("z_plev", 1, 1), ("t_grid", 7, 2), ("mslp", 0, 1), ("z_plev", 1, 3), ("u_grid", 0, 2), ("t_grid", 7, 3))


def test_an_entry_is_a_function_of_its_own_plane_and_pattern(spectral, bc, maps):
    """assim_compute() under MIXED and, on the same state, under the same entries with equal planes adjacent: entry for entry the
    same bits.  Holds the table of distinct planes (csrc/entry_front.hpp) to the order of the caller's list; the mask has two runs."""
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
            model.assim_configure(maps, entries, (1, 0, 1, 1), EVERY, capacity=2, in_loop=False)
            got.append(model.assim_compute().cpu().numpy())  # [E][r]
        assert got[0].shape == (len(MIXED), 3) and np.isfinite(got[0]).all()
        assert np.array_equal(bits(got[0][order]), bits(got[1])), np.argwhere(got[0][order] != got[1]).tolist()
        assert len(np.unique(got[0])) == got[0].size  # (no two entries or members agree)
    finally:
        model.close()
