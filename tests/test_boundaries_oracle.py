"""CPU tier: the oracle as a whole model against the reference Fortran on boundary sets OTHER than the example -- the three sets of
tests/boundary_cases.py (mirrored, icy, patchy) at both start dates, unperturbed, 12 steps (tests/golden/bounds_<set>_<mmdd>_*.npz,
oracle/gen_golden_boundaries.py).  Exact bits, in the manner of tests/test_seasons_oracle.py: the five prognostics at time level 1,
the 21 surface and flux fields the GPU tier compares, and the calendar.  This is what lets tests/test_boundaries_gpu.py take the
oracle as the arbiter on these sets: points filled by fill_missing_values, fractional land nearly everywhere, both sea-ice branches
of the coupler and an orography, a mask and an ice edge the example never shows."""
import os

import numpy as np
import pytest

import band_norms as bn
import boundary_cases as bcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(name, start) for name in bcs.SETS for start in bcs.START_DATES]
MAX_FILE_BYTES = 1 << 20


@pytest.fixture(scope="module")
def bc():
    return np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))


def load(golden_dir, name, start):
    out = {}
    for part in ("spec", "surf"):
        with np.load(bcs.golden_path(golden_dir, name, start, part)) as f:
            out.update({k: f[k] for k in f.files})
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % (c[0], bcs.tag(c[1])))
def test_the_oracle_equals_the_reference_bitwise(oracle, bc, golden_dir, case):
    name, start = case
    gold = load(golden_dir, name, start)
    assert set(gold) == set(bcs.FIELDS + ("cal_ymdhm", "cal_month_idx"))
    for part in ("spec", "surf"):
        assert os.path.getsize(bcs.golden_path(golden_dir, name, start, part)) < MAX_FILE_BYTES
    m = bcs.oracle_model(oracle, bcs.fields(bc, name), start)
    for _ in range(12):
        assert m.step() == 0
    different = []
    for n in bcs.FIELDS:
        got = bcs.get(m, n)
        if n in bcs.SPEC:
            got = got[..., 0]
        assert got.shape == gold[n].shape, (n, got.shape, gold[n].shape)
        if not np.array_equal(got, gold[n]):
            different.append("%s %.3e" % (n, bn.whole_field(got, gold[n])))
    assert not different, "%s from %s: differs from the reference after 12 steps (scaled max error): %s" % (name, start, ", ".join(different))
    ymdhm, month_idx = m.calendar()[:2]
    assert ymdhm == list(gold["cal_ymdhm"]) and month_idx == int(gold["cal_month_idx"])


def test_the_goldens_pin_different_trajectories(golden_dir):
    """Each set's reference run differs from every other's: the files pin six different trajectories."""
    for start in bcs.START_DATES:
        runs = [load(golden_dir, name, start) for name in bcs.SETS]
        for a in range(3):
            for b in range(a + 1, 3):
                assert bn.whole_field(runs[a]["t"], runs[b]["t"]) > 1e-6 and not np.array_equal(runs[a]["sice_am"], runs[b]["sice_am"])
