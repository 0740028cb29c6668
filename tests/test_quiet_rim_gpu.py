"""GPU tier: multi-step calls leave the coefficient blocks beyond the truncation's halo alone for members that hold nothing
there, and nothing a host can see depends on it.

The first step of a multi-step call establishes, on the device, which members have all-zero bits in their dead blocks
(csrc/triangle.hpp, tests/quiet_rim_cases.py); the later steps of the call skip those blocks for those members.  Calls of one
step never skip.  So every test runs 5 steps as ONE call on one model and as five one-step calls on a second model from the same
start, and asks for the same bits in every registry variable of every member, the rim included; option "quiet_rim_members"
reports how many members the call found quiet.

Members start from the reference's init of the example boundary fields with the prognostics of the golden state before step 42,
perturbed per member (band_norms.perturbed_prognostics): zero beyond the triangle, as every state the model produces."""
import numpy as np
import pytest

import band_norms as bn
import quiet_rim_cases as qr
import triangle_cases as tc

pytestmark = pytest.mark.gpu

STEPS = 5
M_SPOT, N_SPOT, LEVEL = 25, 13, 3  # a coefficient of dead block 53 (k = 428, m + n = 38), and the level that is made loud
assert qr.DEAD[M_SPOT, N_SPOT] and qr.DEAD_BLOCKS[(M_SPOT + 31 * N_SPOT) // 8]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir + "/step.npz")


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize % 8 == 0 else a.view(np.uint8)


@pytest.fixture
def pair(spectral, bc, gold):
    """pair(members, options, touch=None, warm=0) -> (the model stepped by ONE call of STEPS steps, the model stepped by STEPS
    calls of one step, the start of both).  Both come from init with the perturbed golden prognostics in every member and `warm`
    single steps; touch(model) then changes the start further.  The models are closed when the test ends, however it ends."""
    from pyspeedy_amd.model import EnsembleModel
    made = []

    def fresh(members, options, touch, warm):
        model = EnsembleModel(spectral, members)
        made.append(model)
        model.set_bc(bc, start_date=(1982, 1, 1, 0, 0))
        for name, value in options:
            model.set_option(name, value)
        for member in range(members):
            for n, a in bn.perturbed_prognostics(gold, member).items():
                model.set(n, a, member)
        for _ in range(warm):
            model.run(1)
        if touch:
            touch(model)
        return model

    def make(members, options, touch=None, warm=0):
        many, single = fresh(members, options, touch, warm), fresh(members, options, touch, warm)
        start = registry(single)
        assert_same_bits(registry(many), start, "start")
        many.run(STEPS)
        for _ in range(STEPS):
            single.run(1)
            assert single.get_option("quiet_rim_members") == -1  # (a call of one step does not look)
        return many, single, start

    yield make
    for model in made:
        model.close()


def registry(model):
    return {n: [model.get(n, i) for i in range(model.nmembers)] for n in model.variables() if n not in ("lon", "lat", "lev")}


def assert_same_bits(got, ref, what):
    assert set(got) == set(ref)
    for n in ref:
        for member, (a, b) in enumerate(zip(got[n], ref[n])):
            assert np.array_equal(bits(a), bits(b)), "%s: %s of member %d differs" % (what, n, member)


def rim_bits(state, member):
    return np.concatenate([bits(state[n][member][qr.DEAD]).ravel() for n in bn.SPEC])


def loud(name, time_level, value, member=4):
    def touch(model):
        a = model.get(name, member)
        spot = (M_SPOT, N_SPOT) + ((LEVEL,) if a.ndim == 4 else ()) + ((time_level,) if a.ndim >= 3 else ())
        assert not bits(a[spot]).any()
        a[spot] = value
        model.set(name, a, member)
        assert np.array_equal(bits(model.get(name, member)), bits(a))
    return touch


@pytest.mark.parametrize("groups", (1, 2))
def test_quiet_members_skip_and_nothing_changes(pair, groups):
    many, single, start = pair(9, (("member_groups", groups), ("block_members", 0)))
    assert not many.config()["fold_geo"] and many.config()["chunks"] == groups and many.config()["rounds"] == 1
    after = registry(many)
    assert_same_bits(after, registry(single), "9 quiet members, %d group(s)" % groups)
    assert many.get_option("quiet_rim_members") == 9
    for member in range(9):
        assert not rim_bits(after, member).any()
    assert not np.array_equal(bits(after["t"][0]), bits(start["t"][0]))  # (the steps were taken)


LOUD = [(n, tl, 1e3) for n in ("vor", "div", "t", "tr", "ps") for tl in (0, 1)]
LOUD += [("tcorh", 0, 1e3), ("qcorh", 0, 1e3), ("t", 0, float("nan")), ("t", 0, -0.0)]


@pytest.mark.parametrize("name,time_level,value", LOUD, ids=["%s-%d-%r" % c for c in LOUD])
def test_one_loud_member_is_carried_as_ever(pair, name, time_level, value):
    # tcorh / qcorh: the first step of a day rewrites both (set_forcing, forcing.f90:15-102: a direct transform, +0.0 beyond the
    # triangle), so what a host sets there lives until midnight only; the call that is to see it starts one step into the day
    warm = 1 if name in ("tcorh", "qcorh") else 0
    many, single, start = pair(9, (("member_groups", 1), ("block_members", 0)), loud(name, time_level, value), warm)
    after = registry(many)
    assert_same_bits(after, registry(single), "member 4 loud in %s" % name)
    assert many.get_option("quiet_rim_members") == 8
    for member in range(9):
        if member != 4:
            assert not rim_bits(after, member).any()
    # the loud member's rim was stepped, not kept (m + n >= 33 feeds itself only, so the triangle does not show it).  Not so for
    # tcorh / qcorh: they enter the tendency, and trfilt, which is 0 beyond the truncation, multiplies every tendency in the time
    # step (time_stepping.f90:164-188) -- the prognostics of that member stay +0.0 there, in the one-step calls as well
    if name in bn.SPEC:
        assert not np.array_equal(rim_bits(after, 4), rim_bits(start, 4))
    else:
        assert not rim_bits(after, 4).any() and bits(after[name][4][qr.DEAD]).any()


def test_the_halo_row_stays_alive(pair, gold):
    def touch(model):
        for n, a in tc.halo_prognostics(gold, 2).items():
            assert a[tc.HALO].any() and not a[tc.L >= 33].any()
            model.set(n, a, 2)
    many, single, start = pair(9, (("member_groups", 1), ("block_members", 0)), touch)
    after = registry(many)
    assert_same_bits(after, registry(single), "member 2 with content at m + n = 32")
    assert many.get_option("quiet_rim_members") == 9
    for n in bn.SPEC:  # the halo row was stepped
        assert not np.array_equal(bits(after[n][2][tc.HALO]), bits(start[n][2][tc.HALO])), n


def test_a_flag_does_not_survive_its_call(pair):
    many, single, _ = pair(9, (("member_groups", 1), ("block_members", 0)))
    assert many.get_option("quiet_rim_members") == 9
    for model in (many, single):
        loud("div", 1, 1e3, member=6)(model)
    many.run(STEPS)
    for _ in range(STEPS):
        single.run(1)
    assert_same_bits(registry(many), registry(single), "junk set between two calls")
    assert many.get_option("quiet_rim_members") == 8


def test_rounds_detect_for_their_own_members(pair):
    options = (("member_groups", 1), ("block_members", 4))
    many, single, _ = pair(16, options, loud("vor", 0, 1e3, member=9))
    assert many.config()["rounds"] == 4  # (member 9 is in the third round)
    assert_same_bits(registry(many), registry(single), "4 rounds of 4 members, member 9 loud")
    assert many.get_option("quiet_rim_members") == 15
