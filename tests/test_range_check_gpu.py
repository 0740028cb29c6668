"""GPU tier: the range check (diagnostics.f90:16-76, csrc/diagnostics_block.hpp) in every form that runs it, pinned to the
REFERENCE's codes at each of its thresholds (tests/golden/range_check.npz, oracle/range_cases.py) and its values to the CPU oracle:

  * diagnostics_kernel on its own: check, check_begin / _end, a deferred check that no step carries, the last step of a checked
    multi-step call, spd_check of the outer boundary
  * the blocks in front of the spectral -> grid launch: check_defer + a step, and every step but the last of run_checked -- whose
    member groups and rounds each pass their own first member
  * spd_parallel_step, which checks every container after its step

The edge cases put both eddy kinetic energies a relative 1e-9 either side of 500 and the global-mean temperature at 180 / 320 K
exactly and one double outside, on every level; a member whose winds blow up during a multi-step call must be reported at the step
at which the oracle's whole model reports it, through the condition that fires there."""
import ctypes as C
import os

import numpy as np
import pytest
import range_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("vor", "div", "t")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir + "/range_check.npz")


@pytest.fixture(scope="module")
def base(golden_dir):
    return RC.base(np.load(golden_dir + "/run.npz"))


@pytest.fixture(scope="module")
def bc():
    with np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz")) as z:
        return {k: z[k] for k in z.files}


def cases(gold, base, which=None, swap=False):
    """the states of the cases `which` (names; all of them by default), in time level 1 -- or in time level 2 over the base
    state's time level 2 (swap: the levels exchanged)"""
    names = [str(n) for n in gold["names"]]
    idx = range(len(names)) if which is None else [names.index(w) for w in which]
    states = [RC.build(base, gold["edits"], i) for i in idx]
    return [RC.swap(s) for s in states] if swap else states, np.array([gold["code"][i] for i in idx]), [names[i] for i in idx]


def load(model, states):
    for i, state in enumerate(states):
        for name, a in zip(FIELDS, state):
            model.set(name, a, i)


def assert_codes(got, code, names, form):
    wrong = [(names[i], int(got[i])) for i in np.nonzero(np.asarray(got) != code)[0]]
    assert not wrong, (form, wrong)


def test_diagnostic_values_equal_the_oracle(spectral, bc, gold, base, oracle):
    """check(tl, with_diag=True), tl = 1 and 2, on 8 members perturbed apart and run 3 steps plus 7 edge cases (in either time
    level): every code equals the oracle's, both kinetic energies within 1e-13 of the oracle's, the temperature bit for bit
    (one multiply on both sides)."""
    from pyspeedy_amd.model import EnsembleModel
    edges, _, _ = cases(gold, base, ["vor_ke_above_l0", "div_ke_below_l7", "t_320_l3", "t_below_180_l5", "zonal_mean_x30",
                                     "two_levels_outside", "other_time_level"])
    P = 8
    M = P + len(edges)
    model = EnsembleModel(spectral, M)
    model.set_bc(bc)
    vor0, t0 = model.get("vor", 0), model.get("t", 0)
    for i in range(1, M):
        rng = np.random.default_rng(300 + i)
        t = t0 * (1.0 + 1e-4 * rng.standard_normal((31, 32, 8, 1)))
        t[0] = t[0].real
        model.set("t", t, i)
        model.set("vor", vor0 * (1.0 + 0.5 * i), i)
    model.run(3)
    load_at = [RC.swap(s) if j % 2 else s for j, s in enumerate(edges)]
    for j, state in enumerate(load_at):
        for name, a in zip(FIELDS, state):
            model.set(name, a, P + j)
    for tl in (1, 2):
        codes, diag = model.check(tl, with_diag=True)
        seen = set()
        for i in range(M):
            rc, ref = RC.oracle_check(oracle, tuple(model.get(n, i) for n in FIELDS), tl)
            got = diag[i].T  # [level, (vorticity KE, divergence KE, temperature)]
            assert codes[i] == rc, (tl, i)
            assert (np.abs(got[:, :2] - ref[:, :2]) <= 1e-13 * np.abs(ref[:, :2])).all(), (tl, i, got[:, :2], ref[:, :2])
            assert np.array_equal(got[:, 2], ref[:, 2]), (tl, i)
            if i < P:
                seen.add(ref.tobytes())
        assert len(seen) == P  # (the perturbed members are 8 different comparisons)
        assert (codes == -2).any() and (codes == 0).any()
    model.close()


def test_every_form_of_the_check_gives_the_reference_codes_at_every_edge(spectral, bc, gold, base):
    """One member per case (69: not a multiple of the 8 workgroups the transform launch's front is padded to): check(1); check(2)
    with the levels exchanged; check_begin / _end of both; check_defer with nothing to carry it; check_defer + run(1) with one
    member group (the check rides in front of the transform launch); check_defer + a call of two steps with the default plan's
    member groups (it goes out on its own first)."""
    from pyspeedy_amd.model import EnsembleModel
    plain, code, names = cases(gold, base)
    swapped, _, _ = cases(gold, base, swap=True)
    M = len(names)
    assert M % 8
    model = EnsembleModel(spectral, M)
    model.set_bc(bc)
    groups = model.config()["chunks"]
    assert groups > 1
    load(model, plain)
    assert_codes(model.check(1), code, names, "check(1)")
    assert_codes(model.check_end(model.check_begin(1)), code, names, "check_begin(1)")
    load(model, swapped)
    assert_codes(model.check(2), code, names, "check(2)")
    assert_codes(model.check_end(model.check_begin(2)), code, names, "check_begin(2)")

    def deferred(form, run, expect_counts):
        alone0, rode0 = model.check_counts()
        token = model.check_defer(2)
        run()
        assert_codes(model.check_end(token), code, names, form)
        alone1, rode1 = model.check_counts()
        assert (alone1 - alone0, rode1 - rode0) == expect_counts, form

    deferred("check_defer, nothing to carry it", lambda: None, (1, 0))
    model.set_option("member_groups", 1)
    deferred("check_defer + run(1)", lambda: model.run(1), (0, 1))
    load(model, swapped)
    model.set_option("member_groups", groups)
    # (a call of one step is issued as one group whatever the plan; one of several steps takes the plan's groups)
    deferred("check_defer + run(2), %d groups" % groups, lambda: model.run(2), (1, 0))
    model.close()


@pytest.mark.parametrize("M", [1, 9])
def test_a_check_riding_in_the_transform_launch_at_the_most_front_padding(spectral, bc, gold, base, M):
    """1 and 9 members: 7 workgroups of the front padding between the check blocks and the transform blocks."""
    from pyspeedy_amd.model import EnsembleModel
    if M == 1:
        rounds = [["div_ke_above_l7"], ["t_320_l0"], ["vor_ke_above_l4"], ["div_ke_below_l1"]]
    else:
        rounds = [["vor_ke_above_l7", "div_ke_below_l6", "t_above_320_l5", "t_180_l4", "div_ke_above_l3", "zonal_mean_x30",
                   "t_below_180_l2", "other_time_level", "vor_ke_below_l0"],
                  ["vor_ke_below_l7", "div_ke_above_l6", "t_320_l5", "t_below_180_l4", "div_ke_below_l3", "base",
                   "t_180_l2", "two_levels_outside", "vor_ke_above_l0"]]
    model = EnsembleModel(spectral, M)
    model.set_bc(bc)
    model.set_option("member_groups", 1)
    for which in rounds:
        states, code, names = cases(gold, base, which, swap=True)
        load(model, states)
        alone0, rode0 = model.check_counts()
        token = model.check_defer(2)
        model.run(1)
        assert_codes(model.check_end(token), code, names, "check_defer + run(1), M = %d" % M)
        assert model.check_counts() == (alone0, rode0 + 1)
    model.close()


# member -> (variable, factor of its eddy coefficients (both time levels, every level) right after init, the kinetic energy that
# leaves the range (0: vorticity, 1: divergence), the step of the call at which the oracle's whole model reports it)
BLOW_UP = {3: ("vor", 240.0, 1, 0), 5: ("div", 30.0, 1, 3), 6: ("vor", 220.0, 0, 1)}


def blown_up(a, factor):
    a = a.copy()
    a[1:] *= factor
    return a


def oracle_failure(oracle, bc, var, factor, nmax):
    """(step at which the oracle's whole model (oracle/orc_model.c) reports the member, its diagnostics there)"""
    cpu = oracle.Model()
    cpu.set_bc(bc)
    assert cpu.init(1982, 1, 1) == 0
    cpu.set(var, blown_up(cpu.get(var), factor))
    for k in range(nmax):
        if cpu.step() != 0:
            rc, diag = RC.oracle_check(oracle, tuple(cpu.get(n) for n in FIELDS), 2)
            assert rc == -2
            return k, diag
    raise AssertionError("the oracle never left the range")


@pytest.fixture(scope="module")
def blow_up_steps(oracle, bc):
    steps = {}
    for member, (var, factor, branch, step) in BLOW_UP.items():
        f, diag = oracle_failure(oracle, bc, var, factor, 6)
        # the condition that fires: this kinetic energy alone, on some level -- the other and the temperature stay inside
        assert (diag[:, branch] > 500.0).any() and (diag[:, 1 - branch] <= 500.0).all(), (member, diag)
        assert ((diag[:, 2] >= 180.0) & (diag[:, 2] <= 320.0)).all(), (member, diag)
        assert f == step, (member, f)
        steps[member] = f
    return steps


@pytest.mark.parametrize("plan", ["one_group", "two_groups", "rounds"])
def test_a_kinetic_energy_blow_up_is_reported_at_the_oracles_step_of_a_checked_call(spectral, bc, blow_up_steps, plan):
    """run_checked(6) on 8 members, three of them blown up right after init so that each leaves the range through one kinetic
    energy (BLOW_UP): member 3 through the divergence at the first step of the call (its check rides in the second step), member
    5 through the divergence at the fourth step, member 6 through the vorticity at the second.  In the plans of
    test_checked_multi_step_call_records_every_steps_range_check: one member group; two (5 and 6 are in the second); rounds of
    two members (5 and 6 in the third and the last round).  Everybody else: -1."""
    from pyspeedy_amd.model import EnsembleModel
    M, K = 8, 6
    model = EnsembleModel(spectral, M)
    model.set_bc(bc)
    for member, (var, factor, _, _) in BLOW_UP.items():
        model.set(var, blown_up(model.get(var, member), factor), member)
    if plan == "one_group":
        model.set_option("member_groups", 1)
    else:
        model.set_option("member_groups", 2)
        model.set_option("block_members", 1 if plan == "rounds" else 0)
    groups, rounds = (1 if plan == "one_group" else 2), (4 if plan == "rounds" else 1)
    alone0, rode0 = model.check_counts()
    failed, accepted = model.run_checked(K)
    alone1, rode1 = model.check_counts()
    assert model.config()["rounds"] == rounds
    assert (rode1 - rode0, alone1 - alone0) == ((K - 1) * groups * rounds, groups * rounds)
    expect = np.full(M, -1)
    for member, f in blow_up_steps.items():
        expect[member] = f
    assert (failed == expect).all(), (plan, failed, expect)
    assert (accepted[:, 0] == np.where(expect < 0, K, expect)).all()
    model.close()


class Driver:
    """the few calls of include/pyspeedy_amd_driver.h these tests make"""

    def __init__(self, lib):
        self.L = lib

    def ok(self, rc):
        assert rc == 0, self.L.spd_last_error()

    def container(self, cnt, bc):
        """boundary fields, init; -> the control container"""
        dates = []
        for ymdhm in ((1982, 1, 1, 0, 0), (1982, 1, 4, 0, 0)):
            d = C.c_int64()
            self.ok(self.L.spd_create_datetime(*ymdhm, C.byref(d)))
            dates.append(d.value)
        ctl = C.c_int64()
        self.ok(self.L.spd_controlparams_init(C.byref(ctl), *dates))
        from pyspeedy_amd.model import BC_MAP
        for name, key in BC_MAP:
            self.set(cnt, name, np.asarray(bc[key], dtype=np.float64))
        code = C.c_int32(99)
        self.ok(self.L.spd_init(cnt, ctl.value, C.byref(code)))
        assert code.value == 0
        return ctl.value

    def set(self, cnt, name, value):
        a = np.ascontiguousarray(np.asarray(value).ravel(order="F"))
        self.ok(self.L.spd_set(cnt, name.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def get(self, cnt, name):
        a = np.zeros(31 * 32 * 8 * 2, dtype=np.complex128)
        self.ok(self.L.spd_get(cnt, name.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes))
        return a.reshape((31, 32, 8, 2), order="F")

    def check(self, cnt):
        code = C.c_int32(99)
        self.ok(self.L.spd_check(cnt, C.byref(code)))
        return code.value

    def parallel_step(self, states, controls):
        n = len(states)
        codes = (C.c_int32 * n)(*([99] * n))
        self.ok(self.L.spd_parallel_step((C.c_int64 * n)(*states), (C.c_int64 * n)(*controls), codes, n))
        return list(codes)


def test_the_outer_boundary_gives_the_reference_codes(spectral, hip_lib, bc, gold, base, blow_up_steps):
    """spd_check (time level 1: the reference's `check`) of 10 containers batched into one device model, each holding a case in
    turn; spd_parallel_step of three containers, one blown up: -2 for that one only, at the oracle's step."""
    drv = Driver(hip_lib)
    n = 10
    cnts = (C.c_int64 * n)()
    drv.ok(hip_lib.spd_modelstate_init_ensemble(cnts, n))
    states = list(cnts)
    for s in states:
        drv.container(s, bc)
    plain, code, names = cases(gold, base)
    for lo in range(0, len(plain), n):
        chunk = range(lo, min(lo + n, len(plain)))
        for s, i in zip(states, chunk):
            for name, a in zip(FIELDS, plain[i]):
                drv.set(s, name, a)
        assert_codes([drv.check(s) for s, _ in zip(states, chunk)], code[lo:lo + n], names[lo:lo + n], "spd_check")
    three = []
    for _ in range(3):
        s = C.c_int64()
        drv.ok(hip_lib.spd_modelstate_init(C.byref(s)))
        three.append(s.value)
    controls = [drv.container(s, bc) for s in three]
    var, factor, _, _ = BLOW_UP[6]
    drv.set(three[1], var, blown_up(drv.get(three[1], var), factor))
    for k in range(blow_up_steps[6]):
        assert drv.parallel_step(three, controls) == [0, 0, 0], k
    assert drv.parallel_step(three, controls) == [0, -2, 0]
    for s in states + three:
        drv.ok(hip_lib.spd_modelstate_close(s))
