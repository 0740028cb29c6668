"""Inside a multi-step call the fused column kernel hands the longwave transmissivities from a shortwave step to the next two
steps as the ten values per column they are made of (surface pressure, cloud cover and top, the clamped humidity of seven levels)
and recomputes them there, instead of storing and re-loading the 32 values of rad_tau2; rad_tau2 itself is stored where a host
can look at it: by the last shortwave step of a call (csrc/physics.hip: COMPACT, csrc/model.hip: step_segment; option
tau_recompute, default on).  The same exp on the same bits: every registry variable of every member must agree in every bit
with the array form -- the separate physics launch (split_dyn) and option tau_recompute = 0 -- after every call, rad_tau2,
tt_rsw and rad_strat_corr included, whatever step of the three-step cycle a call starts and ends on.

Option value 1 (the default) recomputes where 20 members and more step together, value 2 whatever the size: every case runs
with both, so that the small ensembles of these tests go through the compact
form as well as through what a user of their size gets."""
import os

import numpy as np
import pytest
import torch

from pyspeedy_amd.model import EnsembleModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERSISTED = ("rad_tau2", "tt_rsw", "rad_strat_corr")
BOTH = pytest.mark.parametrize("on", [1, 2], ids=["from_20_members", "any_size"])


@pytest.fixture(scope="module")
def boundary():
    bc = np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))
    return {k: bc[k] for k in bc.files}


def _ensemble(spectral, boundary, members, options=(), cfg5=False, co2=False):
    """As bench.py builds its ensemble: the reference's initial state, member i's t_grid += N(0, 0.01 K) with seed i."""
    model = EnsembleModel(spectral, members)
    model.set_bc(boundary, start_date=(1982, 1, 1, 0, 0))
    model.spectral2grid()
    noise = np.stack([np.random.default_rng(i).normal(0.0, 0.01, (96, 48, 8)).transpose(2, 1, 0) for i in range(members)])
    t_grid = model.device_view("t_grid")
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()
    if cfg5:  # BASELINE cfg 5: SPPT on, column physics in fp32
        model.set_sppt(True, seed=11)
        model.set_physics_precision(True)
    if co2:
        model.set_flags(increase_co2=True)
    for name, value in options:
        model.set_option(name, value)
    return model


def _assert_same(a, b, what):
    names = a.variables()
    assert names == b.variables() and len(names) > 80 and all(n in names for n in PERSISTED)
    differing = [(n, i) for n in names for i in range(a.nmembers) if not np.array_equal(a.get(n, i), b.get(n, i))]
    assert not differing, (what, len(differing), differing[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("members,on", [(1, 1), (9, 1), (20, 1), (1, 2), (9, 2), (20, 2)])
def test_default_agrees_bitwise_with_the_separate_physics_launch(spectral, boundary, members, on):
    """Calls of 1, 1, 7, 4, 5, 6 steps from step 0: segments that start on (9, 18), one after (1, 13) and two after (2) a
    shortwave step and end on (12), one after (the one-step call at 1) and two after (8, 17, 23) one.  20 members (two
    member groups of 10) are the smallest ensemble the default recomputes in."""
    compact = _ensemble(spectral, boundary, members, (("tau_recompute", on),) if on != 1 else ())
    array = _ensemble(spectral, boundary, members, (("split_dyn", 1),))
    assert compact.config()["tau_recompute"] == on and not compact.config()["split_dyn"] and array.config()["split_dyn"]
    for call, nsteps in enumerate((1, 1, 7, 4, 5, 6)):
        compact.run(nsteps)
        array.run(nsteps)
        _assert_same(compact, array, "call %d (%d steps), %d members" % (call, nsteps, members))
    assert np.isfinite(compact.get("t", members - 1)).all()
    if members > 1:  # (the members are different: the comparison is not one of copies)
        assert not np.array_equal(compact.get("t", 0), compact.get("t", members - 1))
    compact.close()
    array.close()


@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("storage32", [1, 0])
def test_cfg5_option_on_agrees_bitwise_with_option_off(spectral, boundary, storage32, on):
    which = on
    on = _ensemble(spectral, boundary, 9, (("physics_storage32", storage32), ("tau_recompute", which)), cfg5=True)
    off = _ensemble(spectral, boundary, 9, (("physics_storage32", storage32), ("tau_recompute", 0)), cfg5=True)
    assert on.config()["tau_recompute"] == which and off.config()["tau_recompute"] == 0
    assert on.config()["physics_fp32"] and bool(on.config()["physics_storage32"]) == bool(storage32)
    assert on.device_view("rad_tau2").dtype == (torch.float32 if storage32 else torch.float64)
    for nsteps in (2, 8):
        on.run(nsteps)
        off.run(nsteps)
        _assert_same(on, off, "cfg 5, physics_storage32 = %d, %d steps" % (storage32, nsteps))
    on.close()
    off.close()


@pytest.mark.gpu
@BOTH
def test_rad_tau2_written_between_calls_is_honoured(spectral, boundary, on):
    """Nothing is carried from call to call: two steps without shortwave that open a call read rad_tau2 as the host left it."""
    which = on
    on = _ensemble(spectral, boundary, 9, (("tau_recompute", which),))
    off = _ensemble(spectral, boundary, 9, (("tau_recompute", 0),))
    untouched = _ensemble(spectral, boundary, 9, (("tau_recompute", which),))
    for model in (on, off, untouched):
        model.run(1)
    for model in (on, off):
        view = model.device_view("rad_tau2")
        n = view.numel()
        pattern = 0.5 + 0.45 * torch.sin(torch.arange(n, dtype=torch.float64, device=view.device) * 0.37)
        assert 0.0 <= float(pattern.min()) < 0.1 and 0.9 < float(pattern.max()) <= 1.0
        view.copy_(pattern.reshape(view.shape))
    for model in (on, off, untouched):
        model.run(2)  # steps 1 and 2: no shortwave step in front of them in this call
    _assert_same(on, off, "two steps on the overwritten rad_tau2")
    assert not np.array_equal(on.get("t", 0), untouched.get("t", 0))  # (the overwritten values were used)
    for model in (on, off):
        model.run(5)  # steps 3 ... 7: shortwave at 3 and 6
    _assert_same(on, off, "five more steps")
    for model in (on, off, untouched):
        model.close()


@pytest.mark.gpu
@BOTH
def test_a_day_boundary_with_increasing_co2(spectral, boundary, on):
    """The CO2 absorptivity changes on the first step of a day, which is a shortwave step: the steps that recompute use the
    value their record was made with."""
    on = _ensemble(spectral, boundary, 2, (("tau_recompute", on),), co2=True)
    off = _ensemble(spectral, boundary, 2, (("tau_recompute", 0),), co2=True)
    for model in (on, off):
        model.run(30)
    assert on.current_step == 30
    for model in (on, off):
        model.run(40)  # across step 36
    _assert_same(on, off, "40 steps from step 30")
    on.close()
    off.close()


@pytest.mark.gpu
@BOTH
def test_rounds_follow_the_same_schedule(spectral, boundary, on):
    options = (("member_groups", 1), ("block_members", 1))
    on = _ensemble(spectral, boundary, 4, options + (("tau_recompute", on),))
    off = _ensemble(spectral, boundary, 4, options + (("tau_recompute", 0),))
    assert on.config()["rounds"] == 4 and off.config()["rounds"] == 4
    for model in (on, off):
        model.run(7)
    _assert_same(on, off, "7 steps in 4 rounds")
    on.close()
    off.close()


@pytest.mark.gpu
@BOTH
def test_the_option_shows_and_the_last_shortwave_step_stores_rad_tau2(spectral, boundary, on):
    which = on
    assert _ensemble(spectral, boundary, 1).config()["tau_recompute"] == 1  # (the default)
    on = _ensemble(spectral, boundary, 9, (("tau_recompute", which),))
    off = _ensemble(spectral, boundary, 9, (("tau_recompute", 0),))
    assert on.config()["tau_recompute"] == which and off.config()["tau_recompute"] == 0
    assert on.get_option("tau_recompute") == which and off.get_option("tau_recompute") == 0
    with pytest.raises(ValueError):
        on.set_option("tau_recompute", 3)
    on.run(7)
    before = [on.get("rad_tau2", i) for i in range(9)]
    on.run(7)  # steps 7 ... 13: shortwave at 9 and 12, neither the call's last step
    off.run(14)
    for i in range(9):
        after = on.get("rad_tau2", i)
        assert not np.array_equal(after, before[i])
        assert np.array_equal(after, off.get("rad_tau2", i))
    on.close()
    off.close()
