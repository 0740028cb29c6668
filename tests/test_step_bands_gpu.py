"""GPU tier: the device's model step (spd_model_step_dynamics: spec2grid_table_kernel, physics_kernel with the grid-point
dynamics, grid2spec_table_kernel, spectral_step_kernel) against the CPU oracle PER LEVEL, TIME LEVEL AND TOTAL WAVENUMBER
(tests/band_norms.py), on states in motion and at the time levels and step lengths no other test steps them at.

State: the golden state before step 42 with all five prognostics, both time levels independently, multiplied by
1 + 1e-3 N(0, 1), seed = member index.  Sequences, compared after every call, set_time_step(dt) before each as spd_model_init
does: "startup" = (1, 1, DELT / 2) as a shortwave step, (1, 2, DELT), (2, 2, 2 DELT) -- time_stepping.f90:13-27, which every
other test only runs from the rest state; j1 = j2 = 1 is the one configuration in which the physics' and the dynamics' time
level coincide -- and "leapfrog_delt" = (2, 2, DELT) twice, a leapfrog step with tables for another dt than 2 DELT.  Models: 3
members (geopotential folded into spectral_step_kernel, its EARLY form) and 9 (geopotential_kernel as a launch of its own,
the other form).  Every member is compared with an oracle run of its own and held to
bound = clip(32 nu, 1e-13, 1e-11) per band, nu from 4 one-ulp draws of the oracle's inputs (band_norms.noise_floor; the cap
condition on the inputs is asserted by tests/test_band_norms_cpu.py).  Bands beyond the truncation are exactly zero wherever
the reference's are (band_norms.band_errors says why the temperature's is not).  Figures: profiles/step_bands.txt."""
import numpy as np
import pytest

import band_norms as bn
from test_step_gpu import load_initial

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir + "/step.npz")


def run_on_device(spectral, gold, nmembers, sequence, names):
    """A fresh model of `nmembers` perturbed members through SEQUENCES[sequence] -> [call][member]{name: array}."""
    from pyspeedy_amd.model import EnsembleModel
    model = EnsembleModel(spectral, nmembers)
    load_initial(model, gold)
    for member in range(nmembers):
        for n, a in bn.perturbed_prognostics(gold, member).items():
            model.set(n, a, member)
    calls = []
    for j1, j2, dt, shortwave in bn.SEQUENCES[sequence]:
        model.set_time_step(dt)
        model.step_dynamics(j1, j2, dt, shortwave)
        calls.append([{n: model.get(n, member) for n in names} for member in range(nmembers)])
    config = model.config()
    model.close()
    return calls, config


@pytest.mark.parametrize("sequence", sorted(bn.SEQUENCES))
@pytest.mark.parametrize("nmembers", (3, 9))
def test_every_band_of_every_call_against_the_oracle(spectral, oracle, gold, nmembers, sequence):
    calls, config = run_on_device(spectral, gold, nmembers, sequence, bn.SPEC)
    assert config["fold_geo"] == (nmembers <= 8) and not config["split_dyn"] and config["inv_per_member"] == 77
    failures, worst_ratio, worst_where, worst_whole = [], 0.0, None, 0.0
    for k, call in enumerate(calls):
        whole = dict.fromkeys(bn.SPEC, 0.0)
        for member, got in enumerate(call):
            ref, nu = bn.case(oracle, gold, sequence, member)
            for n in bn.SPEC:
                whole[n] = max(whole[n], bn.whole_field(got[n], ref[k][n]))
                err = bn.band_errors(got[n], ref[k][n])
                rows = bn.worst_bands(err, nu[k][n])
                ratio = rows[0][-3] / rows[0][-1]
                if ratio > worst_ratio:
                    worst_ratio, worst_where = ratio, "member %d, call %d, %s, %s" % (
                        member, k, n, bn.describe(rows[:1], bn.trailing_names(n)))
                if not (err <= bn.bound(nu[k][n])).all():
                    over = int((~(err <= bn.bound(nu[k][n]))).sum())
                    failures.append("member %d, call %d %r, %s: %d of %d bands over the bound; the worst:\n%s" % (
                        member, k, bn.SEQUENCES[sequence][k][:3], n, over, err.size, bn.describe(rows, bn.trailing_names(n))))
        print("%s, %d members, call %d: whole-field max|got - ref| / max|ref| " % (sequence, nmembers, k)
              + ", ".join("%s %.2e" % (n, whole[n]) for n in bn.SPEC))
        worst_whole = max(worst_whole, max(whole.values()))
    print("%s, %d members: worst error / bound %.3f (%s); worst whole-field figure %.2e" % (
        sequence, nmembers, worst_ratio, worst_where, worst_whole))
    assert not failures, "\n".join(failures)


def test_start_up_on_a_moving_state_is_bitwise_in_every_form(spectral, gold, monkeypatch):
    """The forms of the step -- spectral_step_kernel with loads where needed, geopotential_kernel on its own, dynamics and physics
    as two launches, all 91 inverse transforms -- leave every registry variable of every member bitwise as the default does,
    after every call of the start-up sequence on a moving state: with nonzero wind at j1 = j2 = 1, which the form tests of
    tests/test_run_gpu.py (from rest) never see."""
    from pyspeedy_amd.model import SHAPES
    base, config = run_on_device(spectral, gold, 3, "startup", tuple(SHAPES))
    assert config["fold_geo"] and not config["split_dyn"] and config["inv_per_member"] == 77
    assert all(np.abs(base[0][member]["vor"]).max() > 0 for member in range(3))
    assert not np.array_equal(base[0][0]["t"], base[0][1]["t"])
    changed = {"PYSPEEDY_AMD_FOLD_GEO": ("fold_geo", False), "PYSPEEDY_AMD_SPLIT_DYN": ("split_dyn", True),
               "PYSPEEDY_AMD_PRUNE_DEAD": ("inv_per_member", 91)}
    for name, value in (("PYSPEEDY_AMD_SPECTRAL_EARLY", "0"), ("PYSPEEDY_AMD_FOLD_GEO", "0"), ("PYSPEEDY_AMD_SPLIT_DYN", "1"),
                        ("PYSPEEDY_AMD_PRUNE_DEAD", "0")):
        with monkeypatch.context() as mp:
            mp.setenv(name, value)  # read when the model is created
            other, config = run_on_device(spectral, gold, 3, "startup", tuple(SHAPES))
        if name in changed:
            assert config[changed[name][0]] == changed[name][1], (name, config)
        for k in range(len(base)):
            for member in range(3):
                for n in SHAPES:
                    assert np.array_equal(base[k][member][n], other[k][member][n]), (name, k, member, n)
