"""CPU tier (oracle only): the arithmetic of tests/column_bands.py on hand-made arrays; the conditions (a)-(c) on the inputs for
every case that tests/test_physics_bands_gpu.py holds the device to; the census of regimes over those cases; and the
demonstration that the band bound rejects what the whole-field figure lets through.

Observed with 16 draws over all floating-point inputs: worst MARGIN * nu 1.8e-11 (ttend, one band of 48 on physics_sw, 2.1 % of
that output's bands; 1.2e-11 in the same band of physics_nosw), every other output at or below 9.5e-12 (precls), the synthetic
and the edge members at or below 6.3e-12; no integer top changes in any draw.  No case had to be changed.

The planted defects.  Relative defects of 1e-9 in qtend levels 2-3, ttend level 1 and the southernmost zone of evap and ustr, and
1e-20 added to one element of utend at level 3, are each rejected by the band bound in every case.  With the tendency inputs zero
they do NOT all pass the whole-field figure at 1e-12: by the oracle alone that figure is 1.2e-11 ... 1.7e-11 for qtend, 1.9e-11
... 5.1e-11 for ttend, 3.1e-11 ... 1.4e-10 for evap and 3.6e-10 ... 1.0e-9 for ustr (a zone of 8 rows that reaches 60 S holds
0.4 ... 1 of the wind stress maximum, where a single polar row holds a hundredth).  So each defect is planted a second time at
the size the whole-field figure is blind to by construction -- the relative size that moves it to HALF of 1e-12, computed from
the reference: 2.9e-11 ... 4.2e-11 for qtend, 9.9e-12 ... 2.6e-11 for ttend, 3.7e-12 ... 1.6e-11 for evap, 5.0e-13 ... 1.4e-12
for ustr -- and the band bound must reject that smaller defect too, which asks more of the norm than the size of 1e-9 does."""
import numpy as np
import pytest

import column_bands as cb


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------
def hand_made():
    """(96, 48, 3): plane 0 holds zone + 1 everywhere, plane 1 the same with zone 2 zeroed, plane 2 is zero."""
    zone = np.repeat(np.arange(cb.ZONES), cb.ROWS)[None, :] * np.ones((96, 1))
    ref = np.zeros((96, 48, 3))
    ref[:, :, 0] = zone + 1.0
    ref[:, :, 1] = np.where(zone == 2, 0.0, 2.0 * (zone + 1.0))
    return ref


def test_band_membership_and_own_scale():
    ref = hand_made()
    got = ref.copy()
    got[95, 8, 0] += 0.5       # first row of zone 1, last longitude: scale 2
    got[0, 15, 0] -= 0.25      # last row of the same zone: the larger error counts
    got[40, 47, 0] += 6e-3     # the last row of the last zone: scale 6
    got[3, 0, 1] += 1e-6       # zone 0 of plane 1: scale 2
    e = cb.band_errors(got, ref)
    assert e.shape == (3, 6)
    expect = np.zeros((3, 6))
    expect[0, 1], expect[0, 5], expect[1, 0] = 0.25, 1e-3, 0.5e-6
    assert np.allclose(e, expect, rtol=1e-9, atol=0.0) and np.count_nonzero(e) == 3
    # the trailing shape is kept
    assert cb.band_errors(np.zeros((96, 48, 8, 4)), np.zeros((96, 48, 8, 4))).shape == (8, 4, 6)
    assert np.array_equal(cb.band_errors(got[:, :, 0], ref[:, :, 0]), e[0])
    four = np.ones((96, 48, 8, 2))
    moved = four.copy()
    moved[7, 17, 5, 1] += 1e-3
    e4 = cb.band_errors(moved, four)
    assert e4[5, 1, 2] == pytest.approx(1e-3) and np.count_nonzero(e4) == 1
    assert cb.trailing_names("rad_tau2", 4) == ("level", "plane") and cb.trailing_names("ttend", 3) == ("level",)
    assert cb.trailing_names("evap", 3) == ("plane",) and cb.trailing_names("olr", 2) == ()


def test_scale_fall_backs_and_exact_zero():
    ref = hand_made()
    got = ref.copy()
    got[2, 20, 1] = 1e-3   # zone 2 of plane 1: the band's reference is zero -> that plane's maximum over all zones, 12
    e = cb.band_errors(got, ref)
    assert e[1, 2] == pytest.approx(1e-3 / 12.0, rel=1e-12) and np.count_nonzero(e) == 1
    assert cb.zero_bands(ref).sum() == 7 and cb.zero_bands(ref)[1, 2] and cb.zero_bands(ref)[2].all()
    assert cb.nonzero_in_zero_bands(got, ref) == 1 and cb.nonzero_in_zero_bands(ref, ref) == 0
    # plane 2 is zero in every zone: exact
    for value in (1e-300, -1e-300, np.nan):
        got = ref.copy()
        got[50, 33, 2] = value
        e = cb.band_errors(got, ref)
        assert np.isinf(e[2, 4]) and np.count_nonzero(e) == 1
        assert not (e <= cb.bound(np.full_like(e, 1.0))).all()  # no nu admits it
    got = ref.copy()
    got[50, 33, 2] = -0.0
    assert not cb.band_errors(got, ref).any()
    # a NaN in a scaled band stays a NaN, which no bound admits
    got = ref.copy()
    got[1, 1, 0] = np.nan
    e = cb.band_errors(got, ref)
    assert np.isnan(e[0, 0]) and not (e <= cb.bound(np.zeros_like(e))).all()
    assert cb.worst_bands(e, np.zeros_like(e))[0][:2] == (0, 0)


def test_only_the_written_planes_of_hfluxn_count():
    a = np.ones((96, 48, 3))
    assert cb.compared("hfluxn", a).shape == (96, 48, 2) and cb.compared("evap", a).shape == (96, 48, 3)


def test_bound_rule_and_conditions():
    nu = np.array([0.0, 3e-16, 1e-14, 1e-12])
    assert np.array_equal(cb.bound(nu), [1e-13, 1e-13, 32e-14, 32e-12])
    assert (cb.MARGIN, cb.FLOOR, cb.NU_CAP, cb.NU_TIGHT, cb.SHARE_CAP, cb.DRAWS) == (32.0, 1e-13, 1e-10, 1e-11, 0.05, 16)
    quiet = {"x": np.full((8, 6), 1e-15)}
    assert cb.conditions(quiet, 0) == []
    one = {"x": quiet["x"].copy()}
    one["x"][3, 3] = 3e-12                 # 32 nu = 9.6e-11 in 1 band of 48: admissible
    assert cb.conditions(one, 0) == []
    one["x"][3, 3] = 3.2e-12               # 32 nu = 1.02e-10: (a)
    assert len(cb.conditions(one, 0)) == 1 and cb.conditions(one, 0)[0].startswith("(a) x")
    many = {"x": quiet["x"].copy()}
    many["x"][0, :3] = 4e-13               # 32 nu = 1.3e-11 in 3 bands of 48 = 6.25 %: (b)
    assert len(cb.conditions(many, 0)) == 1 and cb.conditions(many, 0)[0].startswith("(b) x")
    many["x"][0, 2] = 1e-15                # 2 of 48 = 4.2 %
    assert cb.conditions(many, 0) == []
    assert cb.conditions(quiet, 2)[0].startswith("(c) 2")


def test_noise_floor_moves_every_floating_point_input_by_an_ulp():
    """run_oracle = the identity: nu is then the perturbation itself, about 2^-52 in every band, zero where the input is zero;
    integer entries are passed on as they are and their changes are counted."""
    rng = np.random.default_rng(0)
    inputs = {"a": rng.uniform(1.0, 2.0, (96, 48, 8)), "b": rng.uniform(1.0, 2.0, (96, 48)), "z": np.zeros((96, 48, 3)),
              "top": rng.integers(1, 9, (96, 48)).astype(np.int32)}
    seen = []

    def run(x):
        seen.append(x)
        out = dict(x)
        if len(seen) == 3:
            out["top"] = x["top"].copy()
            out["top"][4, 4] += 1
        return out

    ref, nu, flipped = cb.noise_floor(run, inputs, 3)
    assert len(seen) == 4 and flipped == 1 and set(nu) == {"a", "b", "z"}
    assert nu["a"].shape == (8, 6) and nu["b"].shape == (6,) and nu["z"].shape == (3, 6)
    for n in ("a", "b"):
        assert ref[n] is inputs[n] and (nu[n] > 0.4 * cb.ULP).all() and nu[n].max() <= 2 * cb.ULP
        for x in seen[1:]:
            assert not np.array_equal(x[n], inputs[n]) and np.abs(x[n] / inputs[n] - 1.0).max() <= 2 * cb.ULP
    assert not nu["z"].any() and all(not x["z"].any() for x in seen) and all(x["top"] is inputs["top"] for x in seen)
    assert not np.array_equal(seen[1]["a"], seen[2]["a"])
    f = cb.ulp_factors(np.random.default_rng(3), (96, 48, 8))
    assert set(np.unique(f)) == {1.0 - cb.ULP, 1.0, 1.0 + cb.ULP}


def test_the_edge_member_holds_the_edges():
    m = cb.edge_member()
    f, snow = m["fmask_land"], m["snowc"]
    for n in cb.SOLAR_IN:
        assert not m[n][:, :16].any() and (m[n][:, 16:] > 0).all()
    assert (f == 0).mean() > 0.4 and (f == 1).mean() > 0.4 and 0.05 < ((f > 0) & (f < 1)).mean() < 0.15
    assert 0.4 < (snow[f > 0] == 0).mean() < 0.6 and (snow[f == 0] > 0).all()
    assert not m["phis0"][f == 0].any() and all(a.flags.f_contiguous and a.dtype == np.float64 for a in m.values())
    z = cb.oracle_inputs(m)
    assert "qg_in" in z and "qg" not in z and not any(z[n].any() for n in cb.TENDENCIES) and m["ttend"].any()


# ---- the cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cb.CASE_NAMES)
def test_conditions_on_the_inputs_hold(oracle, golden_dir, name):
    c = cb.case(oracle, golden_dir, name)
    assert set(c["nu"]) == set(cb.outputs(oracle, c["shortwave"])) and ("cloudc" in c["nu"]) == c["shortwave"]
    for n, v in c["nu"].items():
        r = cb.compared(n, c["ref"][n])
        assert v.shape == r.shape[2:] + (cb.ZONES,) and np.isfinite(r).all() and np.isfinite(v).all(), n
    assert not any(c["inputs"][n].any() for n in cb.TENDENCIES)
    assert ("rad_tau2" in c["inputs"]) == (not c["shortwave"])
    worst = max((cb.MARGIN * float(v.max()), n) for n, v in c["nu"].items())
    share = max((float((cb.MARGIN * v > cb.NU_TIGHT).mean()), n) for n, v in c["nu"].items())
    print("%s: worst MARGIN * nu %.2e (%s); largest share of bands over %.0e: %.1f %% (%s); %s" % (
        name, worst[0], worst[1], cb.NU_TIGHT, 100.0 * share[0], share[1], cb.census_text(c["census"])))
    assert cb.conditions(c["nu"], c["flipped"]) == []


def test_where_the_physics_adds_nothing_the_reference_is_exactly_zero(oracle, golden_dir):
    """u and v above the lowest level and q at the top level: with zero tendency inputs the oracle holds exactly 0 there, so
    the device is compared exactly in those bands."""
    for name in cb.CASE_NAMES:
        ref = cb.case(oracle, golden_dir, name)["ref"]
        for n in ("utend", "vtend"):
            assert not ref[n][:, :, :7].any() and ref[n][:, :, 7].any(), (name, n)
            got = np.array(ref[n], copy=True)
            got[11, 3, 2] = 1e-300
            assert np.isinf(cb.band_errors(got, ref[n])[2, 0])
        assert not ref["qtend"][:, :, 0].any() and ref["qtend"][:, :, 2].any(), name  # (level 2 is zero too on the snapshots)


def test_every_regime_is_present(oracle, golden_dir):
    """Over all cases together (observed: 1070 columns with convective and 39519 with large-scale precipitation of 46080; iptop 2,
    3, 4 and 9 in 6552 ... 17058 columns each; icltop 2, 3, 4, 7 and 9 in 1003 ... 8529 of the 23040 shortwave columns; 4224
    dark columns; 26090 sea, 6836 land and 13154 mixed columns; 37112 with snow, 3460 land or mixed columns without)."""
    total, bare_land = {}, 0
    for name in cb.CASE_NAMES:
        c = cb.case(oracle, golden_dir, name)
        cb.add_census(total, c["census"])
        bare_land += int(((c["inputs"]["fmask_land"] > 0) & (c["inputs"]["snowc"] == 0)).sum())
    print(cb.census_text(total), ", land without snow", bare_land)
    assert total["precnv > 0"] > 300 and total["precls > 0"] > 10000
    for n in cb.TOPS:
        assert sum(1 for count in total[n].values() if count > 500) >= 3, total[n]
    assert total["dark"] > 1000
    assert total["sea"] > 2000 and total["land"] > 2000 and total["mixed"] > 2000
    assert total["snow"] > 10000 and bare_land > 300


# ---- the norm is not blind ----------------------------------------------------------------------------------------------------
ISSUE_SIZE = 1e-9
WHOLE_FIELD_TOL = 1e-12  # what tests/test_physics_gpu.py asks


def _scaled(region):
    def plant(a, size):
        a[region] *= 1.0 + size
    return plant


def _added(a, size):
    a[5, 20, 2] += size


SOUTH = (slice(None), slice(0, cb.ROWS))
# name -> (output, how it is planted, the planted part of the output); levels counted from 1 in the name, from 0 in the slices
PLANTED = {
    "qtend levels 2-3": ("qtend", _scaled((slice(None), slice(None), slice(1, 3))), (slice(None), slice(None), slice(1, 3))),
    "ttend level 1": ("ttend", _scaled((slice(None), slice(None), 0)), (slice(None), slice(None), 0)),
    "evap southernmost zone": ("evap", _scaled(SOUTH), SOUTH),
    "ustr southernmost zone": ("ustr", _scaled(SOUTH), SOUTH),
    "utend level 3 + 1e-20": ("utend", _added, None),
}


def blind_size(ref, region):
    """The relative defect in `region` that moves the whole-field figure to half of WHOLE_FIELD_TOL."""
    return 0.5 * WHOLE_FIELD_TOL * np.abs(ref).max() / np.abs(ref[region]).max()


@pytest.mark.parametrize("name", cb.CASE_NAMES)
def test_band_bound_rejects_what_the_whole_field_figure_lets_through(oracle, golden_dir, name):
    c = cb.case(oracle, golden_dir, name)
    assert cb.conditions(c["nu"], c["flipped"]) == []  # the bound is only as sharp as the inputs are admissible
    failures, _ = cb.verdict(c["ref"], c)
    assert not failures  # the unplanted output passes
    rejected = set()
    for what, (out, plant, region) in PLANTED.items():
        ref = c["ref"][out]
        sizes = [1e-20] if region is None else [ISSUE_SIZE, blind_size(ref, region)]
        verdicts = []
        for size in sizes:
            got = {out: np.array(ref, copy=True)}
            plant(got[out], size)
            assert not np.array_equal(got[out], ref)
            fails, rows = cb.verdict(got, c, [out])
            verdicts.append(bool(fails))
            print("%s, %s at %.2e: whole field %.2e, worst error / bound %.3g" % (name, what, size, rows[0][3], rows[0][1]))
            if size != ISSUE_SIZE:
                assert rows[0][3] <= WHOLE_FIELD_TOL, (what, size, rows[0][3])  # the old figure passes it
            if region is not None:
                assert size <= ISSUE_SIZE
        if all(verdicts):
            rejected.add(what)
    assert rejected == set(PLANTED)
