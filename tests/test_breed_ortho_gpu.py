"""GPU tier: orthonormalised breeding (spd_model_breed_orthogonalize / _gram, csrc/breed.hip) against its definition restated in
numpy (tests/breed_ortho_reference.py; include/pyspeedy_amd.h).  States and rings are compared as bit patterns.

The device's Gram matrix G is held to the arbiter's math.fsum one within 1e-11 sqrt(G_ii G_jj) (34 782 terms, any order of
summation is within 34 782 x 2^-53 = 3.9e-12 of sum |terms| <= sqrt(G_ii G_jj)); everything behind G -- R, C, the ring, the new
states -- is the arbiter's arithmetic on the device's own G, bit for bit.

Shapes: 4 members, control [-1, 0, 0, 0]; 8 members in 2 member groups and 2 rounds, control [-1, 0, 0, 0, 7, 7, 7, -1] (two
families, each with members in another group or round than its control); 20 members, control [-1] + [0] * 19, one breed_apply only
(a family of 19: two full tiles of eight members and a partial one, in the Gram kernel and in the transform).

  1  one breed_apply: G before it, the ring, both time levels of all five variables, what must not move, G after it
  2  a family of one is plain breeding, bit for bit
  3  a member equal to an earlier one of its family: the family breaks there
  4  in-loop run(12), 12 x run(1), the host loop, an unconfigured model moved by the arbiter through get / set, a checked call
     and the quiet rim
  5  breed_orthogonalize(False) is plain breeding again, breed_off() launches nothing
"""
import numpy as np
import pytest

import breed_ortho_reference as ortho
import breed_reference as ref
from test_breed_gpu import (EVERY, RESCALES, SPEC, START, STEPS, bc, bits, differing, elm2, member_state, perturb,  # noqa: F401
                            random_weights, registry, ring_of, same_ring)

pytestmark = pytest.mark.gpu

SHAPES = {"4_members": (4, (), (-1, 0, 0, 0)),
          "8_members_2_groups_2_rounds": (8, (("member_groups", 2), ("block_members", 2)), (-1, 0, 0, 0, 7, 7, 7, -1)),
          "20_members_apply_only": (20, (), (-1,) + (0,) * 19)}


def fresh(spectral, bc, members, options=(), steps=START):
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, members)
    model.set_bc(bc)
    for name, value in options:
        model.set_option(name, value)
    perturb(model)
    model.run(steps)
    return model


def arbiter_event(reg, families, gram, target):
    """What one orthonormalisation makes of the registry `reg`, given the device's own Gram matrix: (the expected registry, the
    expected amplitude and factor rows).  The arbiter's factor and transform, family by family."""
    members = len(reg[SPEC[0]])
    expected = {n: list(v) for n, v in reg.items()}
    amplitude, factor = np.zeros(members), np.ones(members)
    for control, fam in families.items():
        R, c, rank = ortho.factor(gram[np.ix_(fam, fam)], target)
        moved = ortho.transform([member_state(reg, i) for i in fam], member_state(reg, control), c, rank)
        for j, i in enumerate(fam[:rank]):
            amplitude[i], factor[i] = R[j, j], np.float64(target) / np.float64(R[j, j])
            for n in SPEC:
                expected[n][i] = moved[j][n]
    return expected, amplitude, factor


# ---- 1: one breed_apply -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_apply_is_the_definition(spectral, bc, elm2, shape):
    """The target is eight times the first bred member's amplitude: the rounding of the stored X_c + acc (2^-53 |X_c| per
    coefficient, which is not part of CholeskyQR's error form) then stays small against the perturbation that G afterwards measures.
    Both figures (G against fsum; | G' / target^2 - I |_2 against its bound) are printed before they are asserted."""
    members, options, control = SHAPES[shape]
    families = ortho.families(control)
    bred = [i for i in range(members) if control[i] >= 0]
    weights = random_weights(np.random.default_rng(100 + members))
    model = fresh(spectral, bc, members, options)
    try:
        if members == 8:
            assert (model.config()["chunks"], model.config()["rounds"]) == (2, 2)
        before = registry(model)
        model.breed_configure(control, 1.0, EVERY, weights=weights, capacity=2, in_loop=False)
        amplitude0 = model.breed_amplitude().cpu().numpy()
        gram_plain = model.breed_gram().cpu().numpy()  # (with orthogonalisation off)
        target = 8.0 * float(amplitude0[bred[0]])
        model.breed_configure(control, target, EVERY, weights=weights, capacity=2, in_loop=False, orthogonalize=True)
        info = model.breed_info()
        assert (info["orthogonalize"], info["families"], info["largest_family"]) == (True, len(families), max(map(len, families.values())))
        assert (info["bred"], info["taken"], info["applied"]) == (len(bred), 0, 0)
        g = model.breed_gram().cpu().numpy()
        assert np.array_equal(bits(model.breed_amplitude().cpu().numpy()), bits(amplitude0))  # (_compute keeps its meaning)
        assert differing(registry(model), before) == [] and model.breed_info()["taken"] == 0  # (breed_gram writes nothing)
        # G: the same bits with the switch off, symmetric, zero outside the families, the plain amplitude's radicand on the diagonal
        assert g.shape == (members, members) and np.array_equal(bits(g), bits(gram_plain)) and np.array_equal(bits(g), bits(g.T))
        inside = np.zeros((members, members), dtype=bool)
        for fam in families.values():
            inside[np.ix_(fam, fam)] = True
        assert not g[~inside].any() and (np.diag(g)[bred] > 0).all()
        assert np.array_equal(bits(np.sqrt(np.diag(g))), bits(amplitude0))
        worst = 0.0
        for control_of_family, fam in families.items():
            want, _ = ortho.gram([member_state(before, i) for i in fam], member_state(before, control_of_family), weights, elm2)
            scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
            worst = max(worst, float((np.abs(g[np.ix_(fam, fam)] - want) / scale).max()))
        print("%s: G against fsum, worst / sqrt(G_ii G_jj): %.2e" % (shape, worst))
        assert worst < 1e-11
        # the launch
        model.breed_apply()
        after, ring = registry(model), ring_of(model)
        expected, amplitude, factor = arbiter_event(before, families, g, target)
        assert model.breed_info()["taken"] == model.breed_info()["applied"] == 1 and ring["steps"] == [START]
        assert np.array_equal(bits(ring["amplitude"][0]), bits(amplitude)) and np.array_equal(bits(ring["factor"][0]), bits(factor))
        assert (amplitude[bred] > 0).all()  # (nothing broke)
        for i in bred:
            for n in SPEC:
                assert not np.array_equal(bits(expected[n][i]), bits(before[n][i])), (n, i)  # (the case moves the state)
                assert np.array_equal(bits(after[n][i]), bits(expected[n][i])), (n, i, int((bits(after[n][i]) != bits(expected[n][i])).sum()))
                assert np.array_equal(bits(after[n][i][~ref.INSIDE]), bits(before[n][i][~ref.INSIDE])), (n, i)
        assert differing(after, expected) == []  # (the controls, free members and every other registry variable: unchanged)
        # the first member of a family is rescaled as plain breeding would: its amplitude is sqrt(G_11)
        for fam in families.values():
            assert bits(np.float64(ring["amplitude"][0, fam[0]])) == bits(np.float64(amplitude0[fam[0]]))
        # G afterwards: target^2 I, within CholeskyQR's error form 64 r kappa(G) 2^-53 in the spectral norm
        g2 = model.breed_gram().cpu().numpy()
        for fam in families.values():
            r, sub = len(fam), g[np.ix_(fam, fam)]
            bound = 64 * r * np.linalg.cond(sub) * 2.0 ** -53
            err = np.linalg.norm(g2[np.ix_(fam, fam)] / target ** 2 - np.eye(r), 2)
            print("%s: family of %d, kappa(G) = %.3g: | G' / target^2 - I | = %.2e, bound %.2e" % (shape, r, np.linalg.cond(sub), err, bound))
            assert err <= bound, (err, bound)
    finally:
        model.close()


# ---- 2: a family of one -----------------------------------------------------------------------------------------------------------
def test_a_family_of_one_is_plain_breeding(spectral, bc):
    control, got = (-1, 0, -1, 2), []
    weights = random_weights(np.random.default_rng(7))
    for orthogonalize in (False, True):
        model = fresh(spectral, bc, 4, steps=3)
        try:
            model.breed_configure(control, 1e-3, EVERY, weights=weights, capacity=4, orthogonalize=orthogonalize)
            model.breed_apply()
            model.run(6)  # (two in-loop events, at steps 4 and 8)
            got.append((registry(model), ring_of(model), model.breed_info()["applied"]))
        finally:
            model.close()
    assert got[0][2] == got[1][2] == 3 and got[0][1]["steps"] == [3, 4, 8]
    assert differing(got[1][0], got[0][0]) == [] and same_ring(got[1][1], got[0][1])
    assert (got[0][1]["amplitude"][:, [1, 3]] > 0).all()


# ---- 3: the break ---------------------------------------------------------------------------------------------------------------
def test_a_member_equal_to_an_earlier_one_breaks_its_family_there(spectral, bc):
    """Four bred members of control 0 in a norm that sees ln ps only (weight 2, so that G_ij = sum Re D_i Re D_j over m = 0).  Every
    member's ps is the control's except at (m, n) = (0, 1), (0, 2), (0, 3), where the control has 0 and the members the small
    integers (2, 0, 0), (1, 3, 0), (2, 0, 0) -- member 3 equals member 1 there -- and (1, 1, 1): every operation on the way to R is
    exact.  R_11 = 2, R_12 = 1, R_22 = 3, and the third radicand is 4 - 2 * 2 - 0 * 0 = 0: members 3 and 4 keep every bit, members
    1 and 2 are transformed with C = 6 R^-1 = [[3, -1], [0, 2]] in all five variables (their temperatures differ as in every test
    here).  (A duplicate among fields that are not exact may leave a radicand of a few 2^-53 G_jj instead of 0: DESIGN 4k.)"""
    v = {1: (2.0, 0.0, 0.0), 2: (1.0, 3.0, 0.0), 3: (2.0, 0.0, 0.0), 4: (1.0, 1.0, 1.0)}
    model = fresh(spectral, bc, 5, steps=3)
    try:
        ps = model.get("ps", 0)
        ps[0, 1:4, :] = 0.0
        model.set("ps", ps, 0)
        for i, values in v.items():
            mine = ps.copy()
            mine[0, 1:4, 0] = values
            mine[0, 1:4, 1] = values[::-1]  # (time level 2 takes no part in G)
            model.set("ps", mine, i)
        model.breed_configure((-1, 0, 0, 0, 0), 6.0, EVERY, weights={"ps": 2.0}, capacity=1, in_loop=False, orthogonalize=True)
        before = registry(model)
        g = model.breed_gram().cpu().numpy()
        vectors = np.array([v[i] for i in (1, 2, 3, 4)])
        assert np.array_equal(g[1:, 1:], vectors @ vectors.T) and not g[0].any() and not g[:, 0].any()
        model.breed_apply()
        after, ring = registry(model), ring_of(model)
        assert ring["amplitude"][0].tolist() == [0.0, 2.0, 3.0, 0.0, 0.0] and ring["factor"][0].tolist() == [1.0, 3.0, 2.0, 1.0, 1.0]
        expected, amplitude, factor = arbiter_event(before, {0: [1, 2, 3, 4]}, g, 6.0)
        assert amplitude.tolist() == ring["amplitude"][0].tolist()
        assert differing(after, expected) == []
        assert sorted(differing(after, before)) == sorted((n, i) for n in SPEC for i in (1, 2))  # (and only they moved, in all five)
        assert after["ps"][1][0, 1:4, 0].tolist() == [6.0, 0.0, 0.0] and after["ps"][2][0, 1:4, 0].tolist() == [0.0, 6.0, 0.0]
    finally:
        model.close()


# ---- 4, 5: the plans ------------------------------------------------------------------------------------------------------------
class Plans:
    """The runs of one ensemble shape from the same start (step 30), each on a model of its own."""

    def __init__(self, spectral, bc, members, options, control):
        self.members, self.control, self.models = members, control, []
        self.families = ortho.families(control)
        self.bred = [i for i in range(members) if control[i] >= 0]
        self.weights = random_weights(np.random.default_rng(100 + members))

        def start():
            model = fresh(spectral, bc, members, options)
            self.models.append(model)
            return model

        def bred(in_loop=True, orthogonalize=True):
            model = start()
            model.breed_configure(control, self.target, EVERY, weights=self.weights, capacity=8, in_loop=in_loop, orthogonalize=orthogonalize)
            return model

        never = start()
        never.breed_configure(control, 1.0, EVERY, weights=self.weights, capacity=1, in_loop=False)
        self.target = 0.5 * float(never.breed_amplitude()[self.bred[0]])
        never.breed_off()
        never.run(STEPS)
        self.never = registry(never)
        plain = bred(orthogonalize=False)
        plain.run(STEPS)
        self.plain, self.ring_plain = registry(plain), ring_of(plain)
        a = bred()
        a.run(STEPS)
        self.a, self.ring_a, self.info_a = registry(a), ring_of(a), a.breed_info()
        a1 = bred()
        for _ in range(STEPS):
            a1.run(1)
        self.a1, self.ring_a1 = registry(a1), ring_of(a1)
        # the host loop, which also hands the device's Gram matrix of every event to ...
        b, grams = bred(in_loop=False), []
        while b.current_step < START + STEPS:
            b.run(min(EVERY - b.current_step % EVERY, START + STEPS - b.current_step))
            if b.current_step % EVERY == 0:
                grams.append(b.breed_gram().cpu().numpy())
                b.breed_apply()
        self.b, self.ring_b = registry(b), ring_of(b)
        # ... an unconfigured model that the arbiter moves through get / set
        c, rows = start(), []
        while c.current_step < START + STEPS:
            c.run(min(EVERY - c.current_step % EVERY, START + STEPS - c.current_step))
            if c.current_step % EVERY == 0:
                reg = {n: [c.get(n, i) for i in range(members)] for n in SPEC}
                expected, amplitude, factor = arbiter_event(reg, self.families, grams[len(rows)], self.target)
                rows.append((amplitude, factor))
                for i in self.bred:
                    for n in SPEC:
                        c.set(n, expected[n][i], i)
        self.c, self.rows_c = registry(c), rows
        checked = bred()
        self.codes, self.accepted = checked.run_checked(STEPS)
        self.checked, self.ring_checked = registry(checked), ring_of(checked)
        pinned = bred()
        pinned.device_view("phi")  # (the fold pinned off, as tests/test_breed_gpu.py does: the rim looks)
        assert not pinned.config()["fold_geo"]
        pinned.run(STEPS)
        self.rim, self.pinned = pinned.get_option("quiet_rim_members"), registry(pinned)
        off = bred()
        off.breed_orthogonalize(False)
        self.info_plain_again = off.breed_info()
        off.run(STEPS)
        self.plain_again, self.ring_plain_again = registry(off), ring_of(off)
        gone = bred()
        gone.breed_off()
        gone.run(STEPS)
        self.gone, self.info_gone = registry(gone), gone.breed_info()

    def close(self):
        for model in self.models:
            model.close()


@pytest.fixture(scope="module", params=["4_members", "8_members_2_groups_2_rounds"])
def plans(request, spectral, bc):
    p = Plans(spectral, bc, *SHAPES[request.param])
    yield p
    p.close()


def test_in_loop_orthonormalisation_is_the_host_loop_and_the_arbiter(plans):
    assert plans.ring_a["steps"] == list(RESCALES) and plans.info_a["applied"] == plans.info_a["taken"] == len(RESCALES)
    assert {i for n, i in differing(plans.a, plans.never)} == set(plans.bred)  # the case moves every bred member, and nobody else
    later = {i for fam in plans.families.values() for i in fam[1:]}
    assert {i for n, i in differing(plans.a, plans.plain)} == later  # (the first of a family is bred plainly, the others are not)
    assert differing(plans.a1, plans.a) == []  # calls of one step
    assert differing(plans.b, plans.a) == []   # the host loop
    assert differing(plans.c, plans.a) == []   # the arbiter between the calls
    assert same_ring(plans.ring_a1, plans.ring_a) and same_ring(plans.ring_b, plans.ring_a)
    for k, (amplitude, factor) in enumerate(plans.rows_c):
        assert np.array_equal(bits(plans.ring_a["amplitude"][k]), bits(amplitude)), k
        assert np.array_equal(bits(plans.ring_a["factor"][k]), bits(factor)), k
    assert (plans.ring_a["amplitude"][:, plans.bred] > 0).all()  # (no family broke)


def test_a_checked_call_and_the_quiet_rim(plans):
    assert differing(plans.checked, plans.a) == [] and same_ring(plans.ring_checked, plans.ring_a)
    assert (plans.codes == -1).all(), plans.codes  # (no step of any member failed its range check)
    assert (plans.accepted[:, 0] == START + STEPS).all()
    assert plans.rim == plans.members
    assert differing(plans.pinned, plans.a) == []


def test_off_means_plain_breeding_and_then_nothing(plans):
    assert "orthogonalize" not in plans.info_plain_again and plans.info_plain_again["bred"] == len(plans.bred)
    assert differing(plans.plain_again, plans.plain) == [] and same_ring(plans.ring_plain_again, plans.ring_plain)
    assert plans.info_gone == dict(bred=0, every=0, capacity=0, taken=0, held=0, in_loop=False, applied=0)
    assert differing(plans.gone, plans.never) == []
