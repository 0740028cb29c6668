"""GPU tier: breeding (spd_model_breed_*, csrc/breed.hip) against its definition restated in numpy (tests/breed_reference.py).

The definition (include/pyspeedy_amd.h): for a bred member p with control c, A = sqrt(sum weights * E) of the
difference on time level 1, s = target / A, and X_p' = X_c + s (X_p - X_c) on both time levels for m + nn <= 31, every operation
rounded on its own.  States are compared as bit patterns, as tests/test_nudge_gpu.py does; the amplitude against math.fsum of its
34 782 terms within 1e-11 (any order of fewer than 40 000 non-negative terms is within 40 000 x 2^-53 = 4.4e-12 of the exact sum).

Two shapes: 3 members, control = [-1, 0, 0]; 8 members in 2 member groups and 2 rounds, control = [-1, 0, 0, 0, 0, 0, 0, -1], where
bred members sit in another group AND another round than their control.

  1  the arithmetic of one breed_apply: A, s, both time levels of all five variables, and everything that must not move
  2  a bred member equal to its control: A = 0.0, s = 1.0, not one bit moves
  3  plan independence: in-loop run(12), in-loop 12 x run(1), the host loop run(k); breed_apply() and an unconfigured model
     rescaled in numpy through get / set leave the same bits in every registry variable, and the same ring
  4  a checked call leaves the same bits, every code 0, `accepted` as without breeding
  5  the spectra recorder's sample at a rescale step is the spectrum() of the host loop taken BEFORE its breed_apply()
  6  the quiet rim finds every member quiet after a bred multi-step call
  7  breed_off() and a configuration without a bred member launch nothing
  8  twelve bred steps against the CPU oracle stepped with the arbiter's rescale between its steps
"""
import os

import numpy as np
import pytest

import breed_reference as ref

pytestmark = pytest.mark.gpu

SPEC = ref.NAMES
INSIDE = ref.INSIDE
START, STEPS, EVERY = 30, 12, 4
RESCALES = (32, 36, 40)  # 36 is the midnight step


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


@pytest.fixture(scope="module")
def elm2(golden_dir):
    return np.load(os.path.join(golden_dir, "tables.npz"))["elm2"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize % 8 == 0 else a.view(np.uint8)


def registry(model):
    return {n: [model.get(n, i) for i in range(model.nmembers)] for n in model.variables()}


def differing(got, want):
    """the (name, member) pairs of two registries whose bits differ"""
    assert got.keys() == want.keys()
    return [(n, i) for n in want for i in range(len(want[n])) if not np.array_equal(bits(got[n][i]), bits(want[n][i]))]


def perturb(model, seed0=0):
    """as tests/test_nudge_gpu.py: a different temperature per member, factors 1 + 2e-4 N(0, 1), the zonal-mean coefficients keep a
    zero imaginary part"""
    for i in range(model.nmembers):
        f = 1.0 + 2e-4 * np.random.default_rng(seed0 + i).standard_normal((31, 32, 8, 1))
        f[0] = 1.0
        model.set("t", model.get("t", i) * f, i)


def member_state(reg, i):
    return {n: reg[n][i] for n in SPEC}


def random_weights(rng):
    """random weights over the five names, one name (tr) at weight zero"""
    w = {n: rng.uniform(0.1, 1.0, 8) for n in SPEC}
    w["tr"] = np.zeros(8)
    return w


def ring_of(model):
    got = model.breed()
    return dict(amplitude=got["amplitude"].cpu().numpy(), factor=got["factor"].cpu().numpy(), steps=model.breed_steps().tolist(),
                times=model.breed_times())


def same_ring(a, b):
    return (np.array_equal(bits(a["amplitude"]), bits(b["amplitude"])) and np.array_equal(bits(a["factor"]), bits(b["factor"])) and
            a["steps"] == b["steps"] and a["times"] == b["times"])


SPECTRA = ("ke_rot_spectrum", "ke_div_spectrum", "t_spectrum", "q_spectrum", "lnps_spectrum")


class Plans:
    """The runs of one ensemble shape, each on a model of its own from the same start (step 30), kept for the tests below."""

    def __init__(self, spectral, bc, members, options, control):
        from pyspeedy_amd.model import EnsembleModel
        self.members, self.models, self.control = members, [], np.asarray(control, dtype=np.int32)
        self.bred = [int(i) for i in np.flatnonzero(self.control >= 0)]
        rng = np.random.default_rng(100 + members)
        self.weights = random_weights(rng)

        def fresh():
            model = EnsembleModel(spectral, members)
            self.models.append(model)
            model.set_bc(bc)
            for name, value in options:
                model.set_option(name, value)
            perturb(model)
            model.run(START)
            return model

        def bred(in_loop=True, control=self.control):
            model = fresh()
            model.breed_configure(control, self.target, EVERY, weights=self.weights, capacity=8, in_loop=in_loop)
            return model

        # 1: one breed_apply on the state at step 30; the target of every run below is half of the first bred member's amplitude
        one = fresh()
        self.start = registry(one)
        one.breed_configure(self.control, 1.0, EVERY, weights=self.weights, capacity=2, in_loop=False)
        self.amplitude0 = one.breed_amplitude().cpu().numpy()
        assert differing(registry(one), self.start) == [] and one.breed_info()["taken"] == 0  # (breed_amplitude writes nothing)
        self.target = 0.5 * float(self.amplitude0[self.bred[0]])
        one.breed_configure(self.control, self.target, EVERY, weights=self.weights, capacity=2, in_loop=False)
        self.info_one_before = one.breed_info()
        one.breed_apply()
        self.one, self.ring_one, self.info_one = registry(one), ring_of(one), one.breed_info()
        # never bred: plain and checked
        never = fresh()
        self.config = never.config()
        self.codes_never, self.accepted_never = never.run_checked(STEPS)
        self.never = registry(never)
        # A: in-loop, one call, with the spectra recorder on
        a = bred()
        a.spectra_configure(SPECTRA, EVERY, 4)
        assert differing(registry(a), self.start) == []
        a.run(STEPS)
        self.a, self.ring_a, self.info_a = registry(a), ring_of(a), a.breed_info()
        self.spectra_a = {n: a.spectra(n).cpu().numpy() for n in SPECTRA}
        self.spectra_steps_a = a.spectra_steps().tolist()
        # A': in-loop, calls of one step
        a1 = bred()
        for _ in range(STEPS):
            a1.run(1)
        self.a1, self.ring_a1, self.info_a1 = registry(a1), ring_of(a1), a1.breed_info()
        # B: the host loop run(k); breed_apply(), with spectrum() taken before each breed_apply()
        b = bred(in_loop=False)
        self.spectrum_b = []
        while b.current_step < START + STEPS:
            b.run(min(EVERY - b.current_step % EVERY, START + STEPS - b.current_step))
            if b.current_step % EVERY == 0:
                got = b.spectrum(SPECTRA)
                self.spectrum_b.append({n: got[n].cpu().numpy() for n in SPECTRA})
                b.breed_apply()
        self.b, self.ring_b, self.info_b = registry(b), ring_of(b), b.breed_info()
        # C: an unconfigured model rescaled in numpy through get / set, s from A's ring
        c = fresh()
        event = 0
        while c.current_step < START + STEPS:
            c.run(min(EVERY - c.current_step % EVERY, START + STEPS - c.current_step))
            if c.current_step % EVERY == 0:
                for i in self.bred:
                    s = self.ring_a["factor"][event, i]
                    for n in SPEC:
                        c.set(n, ref.rescale_variable(c.get(n, i), c.get(n, int(self.control[i])), s), i)
                event += 1
        self.c = registry(c)
        # a checked call
        checked = bred()
        self.codes, self.accepted = checked.run_checked(STEPS)
        self.checked, self.ring_checked = registry(checked), ring_of(checked)
        # the quiet rim: the fold pinned off (a view of phi does that; a call that folds the geopotential does not look)
        pinned = bred()
        pinned.device_view("phi")
        assert not pinned.config()["fold_geo"]
        pinned.run(STEPS)
        self.rim, self.pinned = pinned.get_option("quiet_rim_members"), registry(pinned)
        # off means off: a configuration switched off again, and one without a bred member
        off = bred()
        off.breed_off()
        off.run(STEPS)
        self.off, self.info_off = registry(off), off.breed_info()
        nobody = bred(control=np.full(members, -1))
        nobody.run(STEPS)
        nobody.breed_apply()
        self.nobody, self.info_nobody = registry(nobody), nobody.breed_info()

    def close(self):
        for model in self.models:
            model.close()


@pytest.fixture(scope="module", params=[(3, (), (-1, 0, 0)),
                                        (8, (("member_groups", 2), ("block_members", 2)), (-1, 0, 0, 0, 0, 0, 0, -1))],
                ids=["3_members", "8_members_2_groups_2_rounds"])
def plans(request, spectral, bc):
    members, options, control = request.param
    p = Plans(spectral, bc, members, options, control)
    yield p
    p.close()


def test_the_plan_is_the_one_the_case_is_about(plans):
    if plans.members == 3:
        assert (plans.config["chunks"], plans.config["rounds"]) == (1, 1)
    else:  # bred members 2 ... 6 lie in another round or another group than member 0
        assert (plans.config["chunks"], plans.config["rounds"]) == (2, 2)
    assert (START + STEPS) % EVERY != 0 and START % EVERY != 0  # (the call neither starts nor ends at a rescale step)


# ---- 1: the arithmetic of one launch ---------------------------------------------------------------------------------------
def test_apply_is_the_definition(plans, elm2):
    before, after, ring = plans.start, plans.one, plans.ring_one
    assert plans.info_one_before == dict(bred=len(plans.bred), every=EVERY, capacity=2, taken=0, held=0, in_loop=False, applied=0)
    assert plans.info_one["taken"] == plans.info_one["applied"] == 1 and ring["steps"] == [START]
    assert ring["amplitude"].shape == ring["factor"].shape == (1, plans.members)
    expected = {n: list(v) for n, v in before.items()}
    for i in range(plans.members):
        a, s = ring["amplitude"][0, i], ring["factor"][0, i]
        if i not in plans.bred:
            assert a == 0.0 and s == 1.0, i
            continue
        xp, xc = member_state(before, i), member_state(before, int(plans.control[i]))
        want = ref.amplitude(xp, xc, plans.weights, elm2)
        print("member %d: A = %.17g, against fsum %.2e" % (i, a, abs(a / want - 1.0)))
        assert want > 0 and abs(a / want - 1.0) < 1e-11, (i, a, want)
        assert np.array_equal(bits(a), bits(plans.amplitude0[i]))  # (breed_amplitude: the same number)
        assert bits(np.float64(s)) == bits(np.float64(plans.target) / np.float64(a)), (i, s)
        moved = ref.rescale(xp, xc, np.float64(s))
        for n in SPEC:
            assert not np.array_equal(bits(moved[n]), bits(before[n][i])), n  # (the case moves the state)
            assert np.array_equal(bits(after[n][i]), bits(moved[n])), (n, i, int((bits(after[n][i]) != bits(moved[n])).sum()))
            # not one bit of a coefficient with m + nn >= 32 moved, on either time level
            assert np.array_equal(bits(after[n][i][~INSIDE]), bits(before[n][i][~INSIDE])), (n, i)
            expected[n][i] = moved[n]
    assert abs(ring["factor"][0, plans.bred[0]] - 0.5) < 1e-12  # (the target is half of that member's amplitude)
    assert differing(after, expected) == []  # (the controls, the free member and every other registry variable: unchanged)


# ---- 2: the degenerate member ------------------------------------------------------------------------------------------------
def test_a_member_equal_to_its_control_is_left_alone(spectral, bc):
    from pyspeedy_amd import SpeedyHipError
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, 3)
    try:
        model.set_bc(bc)
        perturb(model)
        model.run(3)
        for n in SPEC:  # member 2 becomes its control, bit for bit
            model.set(n, model.get(n, 0), 2)
        with pytest.raises(SpeedyHipError, match="no breeding configured"):
            model.breed_apply()
        with pytest.raises(SpeedyHipError, match=r"the control of member 2 \(1\) is itself bred"):
            model.breed_configure([-1, 0, 1], 1.0, EVERY)
        with pytest.raises(SpeedyHipError, match="member 1 is its own control"):
            model.breed_configure([-1, 1, 0], 1.0, EVERY)
        with pytest.raises(SpeedyHipError, match=r"the control of member 1 \(3\) is out of range"):
            model.breed_configure([-1, 3, 0], 1.0, EVERY)
        assert model.breed_info()["bred"] == 0
        model.breed_configure([-1, 0, 0], 1.0, EVERY, weights="total_energy", capacity=1, in_loop=False)
        before = registry(model)
        model.breed_apply()
        after, ring = registry(model), ring_of(model)
        assert ring["amplitude"][0, 2] == 0.0 and ring["factor"][0, 2] == 1.0
        assert ring["amplitude"][0, 1] > 0.0 and ring["factor"][0, 1] == 1.0 / ring["amplitude"][0, 1]
        assert [(n, i) for n, i in differing(after, before) if i != 1] == []
        assert sorted(n for n, i in differing(after, before)) == sorted(SPEC)  # (member 1 moved in all five)
        # the ring keeps the last `capacity` events
        model.breed_apply()
        assert model.breed_info()["taken"] == 2 and model.breed_info()["held"] == 1
        # the rescaled member stands at the target: the stored state rounds at 2^-53 of coefficients up to 1e3 times the
        # perturbation's, far below 1e-9
        assert abs(ring_of(model)["amplitude"][0, 1] - 1.0) < 1e-9
        model.breed_reset()
        assert model.breed_info()["taken"] == 0 and model.breed()["amplitude"].shape == (0, 3)
    finally:
        model.close()


# ---- 3 - 7: the plans --------------------------------------------------------------------------------------------------------
def test_in_loop_breeding_does_not_depend_on_the_plan_and_is_the_host_loop(plans):
    assert plans.ring_a["steps"] == list(RESCALES)
    assert [(t.hour, t.minute) for t in plans.ring_a["times"]] == [(21, 20), (0, 0), (2, 40)]
    moved = differing(plans.a, plans.never)
    assert {i for n, i in moved} == set(plans.bred)  # the case moves every bred member, and nobody else
    assert differing(plans.a1, plans.a) == []  # calls of one step
    assert differing(plans.b, plans.a) == []   # the host loop
    assert differing(plans.c, plans.a) == []   # numpy between the calls
    assert same_ring(plans.ring_a1, plans.ring_a) and same_ring(plans.ring_b, plans.ring_a)
    for info in (plans.info_a, plans.info_a1, plans.info_b):
        assert info["applied"] == info["taken"] == len(RESCALES) and info["bred"] == len(plans.bred)
    # every event: the amplitude of a bred member has grown from the target, its factor is target / A; the others show 0 and 1
    for i in range(plans.members):
        a, s = plans.ring_a["amplitude"][:, i], plans.ring_a["factor"][:, i]
        if i in plans.bred:
            assert (a > 0).all() and np.array_equal(bits(s), bits(np.float64(plans.target) / a))
            assert (a[1:] != plans.target).all()  # (four steps moved the amplitude away from the target)
        else:
            assert not a.any() and (s == 1.0).all()


def test_a_checked_call_leaves_the_same_bits_and_accepts_every_step(plans):
    assert differing(plans.checked, plans.a) == []
    assert same_ring(plans.ring_checked, plans.ring_a)
    assert (plans.codes == -1).all(), plans.codes  # (no step of any member failed its range check)
    assert (plans.codes_never == -1).all()
    assert np.array_equal(plans.accepted, plans.accepted_never) and (plans.accepted[:, 0] == START + STEPS).all()


def test_a_recorder_sees_the_state_the_rescale_step_left(plans):
    assert plans.spectra_steps_a == list(RESCALES) and len(plans.spectrum_b) == len(RESCALES)
    for n in SPECTRA:
        for k in range(len(RESCALES)):
            got, want = plans.spectra_a[n][:, k], plans.spectrum_b[k][n]
            assert want.any() and np.array_equal(bits(got), bits(want)), (n, k)


def test_the_quiet_rim_finds_every_member_quiet_after_a_bred_call(plans):
    assert plans.rim == plans.members
    assert differing(plans.pinned, plans.a) == []


def test_off_means_off(plans):
    assert plans.info_off == dict(bred=0, every=0, capacity=0, taken=0, held=0, in_loop=False, applied=0)
    assert plans.info_nobody == dict(bred=0, every=EVERY, capacity=8, taken=0, held=0, in_loop=True, applied=0)
    assert differing(plans.off, plans.never) == []
    assert differing(plans.nobody, plans.never) == []


# ---- 8: against the CPU oracle ------------------------------------------------------------------------------------------------
def test_twelve_bred_steps_against_the_oracle(spectral, oracle, bc, elm2):
    """Control and one bred member, 12 steps from `init`, a rescale every 4 steps (at 4, 8 and 12) in the total-energy norm to half of
    the initial amplitude.  Two oracle models (oracle/orc_model.c) are stepped side by side with the arbiter's rescale -- its own
    fsum amplitude, its own s -- applied through get / set; the device runs the same as ONE call.  The criterion is the one of
    tests/test_model_vs_oracle_gpu.py at this step count: every one of vor, div, t, tr, ps of both members within 1e-11 of its max
    norm.  The amplitudes of the two sides are printed, not held to a bound of their own: the perturbation is about 1e-4 of the
    state, so a state error of 1e-11 may show as 1e-7 in A.  Observed worst: 1.9e-14 (div of the control; vor 8.2e-15, t, tr and ps
    below 1e-15), the amplitudes within 2e-13."""
    from pyspeedy_amd import breed_weights
    from pyspeedy_amd.model import EnsembleModel
    weights = breed_weights("total_energy")
    factor = 1.0 + 2e-4 * np.random.default_rng(8).standard_normal((31, 32, 8, 1))
    factor[0] = 1.0
    cpu = [oracle.Model(), oracle.Model()]
    for model in cpu:
        model.set_bc(bc)
        assert model.init(1982, 1, 1) == 0
    cpu[1].set("t", cpu[1].get("t") * factor)
    state = lambda model: {n: model.get(n) for n in SPEC}  # noqa: E731
    target = 0.5 * ref.amplitude(state(cpu[1]), state(cpu[0]), weights, elm2)
    model = EnsembleModel(spectral, 2)
    try:
        model.set_bc(bc)
        model.set("t", model.get("t", 1) * factor, 1)
        model.breed_configure([-1, 0], target, EVERY, weights=weights, capacity=3)
        model.run(12)
        assert model.breed_info()["applied"] == 3
        got = [{n: model.get(n, i) for n in SPEC} for i in range(2)]
        ring = ring_of(model)
    finally:
        model.close()
    amplitudes = []
    for step in range(1, 13):
        assert cpu[0].step() == 0 and cpu[1].step() == 0
        if step % EVERY == 0:
            xp, xc = state(cpu[1]), state(cpu[0])
            a = ref.amplitude(xp, xc, weights, elm2)
            amplitudes.append(a)
            for n, v in ref.rescale(xp, xc, np.float64(target) / np.float64(a)).items():
                cpu[1].set(n, v)
    print("amplitudes, device against the oracle's:", [abs(x / y - 1.0) for x, y in zip(ring["amplitude"][:, 1], amplitudes)])
    worst = {}
    for i in range(2):
        for n in SPEC:
            want = cpu[i].get(n)
            worst[n, i] = float(np.abs(got[i][n].reshape(want.shape) - want).max() / np.abs(want).max())
    print("bred model against the oracle after 12 steps, error / max norm:", worst)
    assert max(worst.values()) < 1e-11, worst
