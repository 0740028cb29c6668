"""The step's grid -> spectral launch forms the 40 flux and kinetic-energy products itself (csrc/staged_products.hpp, the
product table of model.hip: build_tables) and the fused column kernel no longer stores them.  The separate dynamics and physics
launches (option split_dyn) keep the stores and the plain table.  The arithmetic is the same expressions on the same inputs, so
the two must agree in every bit: every registry variable of every member, after the start-up step, after one more one-step call
and after a multi-step call (shortwave and non-shortwave steps), at 1 member (folded / early forms), 9 members (plain forms
above 8 members, quiet-rim detect and skip) and 20 members (two member groups)."""
import os

import numpy as np
import pytest
import torch

from pyspeedy_amd.model import EnsembleModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def boundary():
    bc = np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))
    return {k: bc[k] for k in bc.files}


def _ensemble(spectral, boundary, members, split):
    """As bench.py builds its ensemble: the reference's initial state, member i's t_grid += N(0, 0.01 K) with seed i."""
    model = EnsembleModel(spectral, members)
    model.set_bc(boundary, start_date=(1982, 1, 1, 0, 0))
    model.spectral2grid()
    noise = np.stack([np.random.default_rng(i).normal(0.0, 0.01, (96, 48, 8)).transpose(2, 1, 0) for i in range(members)])
    t_grid = model.device_view("t_grid")
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()
    if split:
        model.set_option("split_dyn", 1)
    return model


@pytest.mark.gpu
@pytest.mark.parametrize("members", [1, 9, 20])
def test_staged_products_agree_bitwise_with_stored_products(spectral, boundary, members):
    staged = _ensemble(spectral, boundary, members, split=False)
    stored = _ensemble(spectral, boundary, members, split=True)
    assert staged.config()["forward_table"] == "products" and stored.config()["forward_table"] == "plain"
    assert staged.config()["forward_table"] != stored.config()["forward_table"]  # (the switch did switch something)
    assert not staged.config()["split_dyn"] and stored.config()["split_dyn"]
    names = staged.variables()
    assert names == stored.variables() and len(names) > 80
    for call, nsteps in enumerate((1, 1, 7)):
        staged.run(nsteps)
        stored.run(nsteps)
        differing = [(n, i) for n in names for i in range(members) if not np.array_equal(staged.get(n, i), stored.get(n, i))]
        assert not differing, ("call %d (%d steps), %d members" % (call, nsteps, members), len(differing), differing[:5])
    assert np.isfinite(staged.get("t", members - 1)).all()
    if members > 1:  # (the members are different: the comparison is not one of copies)
        assert not np.array_equal(staged.get("t", 0), staged.get("t", members - 1))
    staged.close()
    stored.close()
