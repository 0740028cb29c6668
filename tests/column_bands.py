"""Helper of the column-band tests (not a test): errors of the column physics' outputs per latitude zone and level or plane, the
oracle's own rounding sensitivity in the same norm, and the cases that tests/test_column_bands_cpu.py (oracle only) and
tests/test_physics_bands_gpu.py (device against oracle) share.

A whole-field figure max|got - ref| / max|ref| over a [lon][lat][level] array is blind wherever the output is small next to its
maximum: the physics' own temperature tendency at the top level is a few percent of the one near the surface, the stratospheric
moisture tendency a few thousandths of the lowest level's, and a polar row of a surface flux a hundredth of the tropical maximum.
Here a band is one latitude zone (ZONES = 6 zones of ROWS = 8 Gaussian rows, south to north) times one trailing index of the
output -- the level of a [.., 8] output, the surface-type plane of a [.., 3] output, (level, plane) of rad_st4a and rad_tau2, the
plane of rad_flux and rad_strat_corr, nothing for a 2-D output -- over all 96 longitudes.  Only planes 0-1 of hfluxn are compared
(the reference never writes plane 2), cloudc and clstr on shortwave steps only.  Every band is scaled by its own max|ref|; where
that is exactly zero, by the maximum of the same trailing index over all zones; where that is zero too the band is compared
exactly: the device must hold 0.0 there, the error is inf otherwise.

The bound comes from the reference: nu, the largest change of the oracle's result in that band when every floating-point input
(the six state fields, the surface and shortwave inputs and, on steps without shortwave, the persisted radiation state) moves by
at most one ulp, times a margin,

    bound = max(MARGIN * nu, FLOOR)

MARGIN = 32 and FLOOR = 1e-13 with the reasoning of tests/band_norms.py: nu seeds ONE rounding per input, the device differs by one
rounding at every contracted multiply-add and by its own exp / log / pow; the floor keeps bands whose nu is an ulp from demanding
sub-ulp agreement.  Single rows instead of zones are too few columns: near a threshold of the moist schemes one column then owns a
band and the oracle's own sensitivity there reaches 1e-10.  No band and no column is left out.

The inputs must be admissible by the oracle alone (`conditions`; asserted before any device result is looked at): (a) MARGIN * nu
<= NU_CAP = 1e-10 in every band, (b) per output at most SHARE_CAP = 5 % of the bands have MARGIN * nu > NU_TIGHT = 1e-11, (c) no
integer top (iptop, and icltop on shortwave steps) changes in any draw.  These are conditions on the cases, not tolerances.

The cases run with the four tendency inputs EXACTLY ZERO, so the tendency outputs are the physics' own tendencies (and u, v above
the lowest level and q at the top level exactly zero); the addition onto a non-zero input is the subject of
tests/test_physics_gpu.py and tests/test_physics_replay_gpu.py."""
import numpy as np

ZONES, ROWS = 6, 8
MARGIN, FLOOR = 32.0, 1e-13
NU_CAP, NU_TIGHT, SHARE_CAP = 1e-10, 1e-11, 0.05
DRAWS = 16
ULP = 2.0 ** -52

TENDENCIES = ("utend", "vtend", "ttend", "qtend")
SHORTWAVE_ONLY = ("cloudc", "clstr")
PLANES = {"hfluxn": 2}  # compared planes of an output of which the reference does not write all
TOPS = ("iptop", "icltop")
SOLAR_IN = ("flux_solar_in", "flux_ozone_upper", "flux_ozone_lower")


def outputs(oracle, shortwave):
    """Names of the floating-point outputs compared on a step of that kind."""
    names = TENDENCIES + tuple(oracle.PHYS_OUT_SHAPES) + tuple(oracle.PHYS_PERSIST_SHAPES) + tuple(oracle.PHYS_DIAG_F)
    return tuple(n for n in names if shortwave or n not in SHORTWAVE_ONLY)


def tops(shortwave):
    return TOPS if shortwave else TOPS[:1]


def compared(name, a):
    """The part of output `name` (reference host layout (96, 48[, ...])) that is compared."""
    a = np.asarray(a)
    return a[:, :, :PLANES[name]] if name in PLANES else a


def whole_field(got, ref):
    """The figure the older tests use: max|got - ref| / max|ref| over the whole array."""
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _zone_max(a):
    """(96, 48, ...) -> [ZONES][J]: the maximum over the longitudes and the rows of a zone, per flattened trailing index."""
    return a.reshape(96, ZONES, ROWS, -1).max(axis=(0, 2))


def band_scale(ref):
    """-> (scale [trailing..., ZONES], exact [trailing..., ZONES]): the band's own max|ref|, or the maximum of the trailing index over
    all zones where that is zero; exact marks the bands where both are zero (scale 1 there)."""
    ref = np.asarray(ref, dtype=np.float64)
    mag = _zone_max(np.abs(ref))
    slab = mag.max(axis=0, keepdims=True)
    exact = np.broadcast_to(slab == 0.0, mag.shape)
    scale = np.where(mag > 0.0, mag, np.where(exact, 1.0, slab))
    shape = ref.shape[2:] + (ZONES,)
    return scale.T.reshape(shape), exact.T.reshape(shape)


def band_errors(got, ref):
    """got, ref: (96, 48[, ...]) in reference host layout -> float array [trailing shape..., ZONES]: max|got - ref| over the band /
    scale (band_scale); 0.0 or inf in the bands that are compared exactly.  A NaN of the device stays a NaN, which no bound
    admits."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and got.shape[:2] == (96, ZONES * ROWS), (got.shape, ref.shape)
    scale, exact = band_scale(ref)
    shape = ref.shape[2:] + (ZONES,)
    diff = _zone_max(np.abs(got - ref)).T.reshape(shape)
    held = _zone_max(np.where(np.isnan(got), np.inf, np.abs(got))).T.reshape(shape)
    return np.where(exact, np.where(held > 0.0, np.inf, 0.0), diff / scale)


def zero_bands(ref):
    """[trailing shape..., ZONES] bool: the bands in which the reference is exactly zero (whatever the other zones hold)."""
    ref = np.asarray(ref, dtype=np.float64)
    return (_zone_max(np.abs(ref)) == 0.0).T.reshape(ref.shape[2:] + (ZONES,))


def nonzero_in_zero_bands(got, ref):
    """Number of bands in which the reference is exactly zero and got is not (a NaN counts)."""
    got = np.asarray(got, dtype=np.float64)
    held = _zone_max(np.where(np.isnan(got), np.inf, np.abs(got))).T.reshape(got.shape[2:] + (ZONES,))
    return int((zero_bands(ref) & (held > 0.0)).sum())


def ulp_factors(rng, shape):
    """1 + 2^-52 * r with r in {-1, 0, 1} per element."""
    return 1.0 + ULP * rng.integers(-1, 2, size=shape).astype(np.float64)


def noise_floor(run_oracle, inputs, draws=DRAWS):
    """The reference's own rounding sensitivity nu.  run_oracle(inputs) -> dict name -> array, all outputs of oracle.physics on
    `inputs` (a dict of its arguments: state, surface and shortwave inputs, zero tendencies and -- on a step without shortwave --
    the persisted radiation state).  -> (reference, nu, flipped): the result for the inputs as they are; per floating-point output
    the largest band_errors between it and `draws` results, in each of which every element of every floating-point input is
    multiplied by ulp_factors from default_rng(draw); and the number of columns in which an integer top differs, summed over tops
    and draws.  Only the oracle runs here (about 10 ms a call)."""
    reference = run_oracle(inputs)
    names = [n for n, a in reference.items() if np.asarray(a).dtype.kind == "f"]
    integer = [n for n, a in reference.items() if np.asarray(a).dtype.kind == "i"]
    nu = {n: np.zeros(compared(n, reference[n]).shape[2:] + (ZONES,)) for n in names}
    flipped = 0
    for draw in range(draws):
        rng = np.random.default_rng(draw)
        moved = {}
        for n, a in inputs.items():
            a = np.asarray(a)
            moved[n] = a * ulp_factors(rng, a.shape) if a.dtype.kind == "f" else a
        out = run_oracle(moved)
        for n in names:
            nu[n] = np.maximum(nu[n], band_errors(compared(n, out[n]), compared(n, reference[n])))
        flipped += sum(int((out[n] != reference[n]).sum()) for n in integer)
    return reference, nu, flipped


def bound(nu):
    return np.maximum(MARGIN * np.asarray(nu), FLOOR)


def conditions(nu, flipped):
    """-> list of texts, one per broken condition (a)-(c) on the inputs; nu: name -> array."""
    broken = []
    for n, v in nu.items():
        worst = MARGIN * float(np.max(v))
        if not worst <= NU_CAP:
            broken.append("(a) %s: MARGIN * nu reaches %.3e > %.0e" % (n, worst, NU_CAP))
        share = float((MARGIN * v > NU_TIGHT).mean())
        if not share <= SHARE_CAP:
            broken.append("(b) %s: MARGIN * nu > %.0e in %.1f %% of the %d bands" % (n, NU_TIGHT, 100.0 * share, v.size))
    if flipped:
        broken.append("(c) %d columns changed an integer top under one-ulp moves of the inputs" % flipped)
    return broken


def trailing_names(name, ndim):
    """Names of the trailing indices of an output of `ndim` dimensions in host layout."""
    if ndim == 4:
        return ("level", "plane")
    if ndim == 3:
        return ("plane",) if name in ("slru", "ustr", "vstr", "shf", "evap", "hfluxn", "rad_flux", "rad_strat_corr") else ("level",)
    return ()


def worst_bands(err, nu, count=5):
    """[(trailing index..., zone, error, nu, bound)] of the `count` bands with the largest error / bound, worst first (a NaN
    first of all)."""
    b = bound(nu)
    ratio = np.where(np.isnan(err), np.inf, err / b)
    order = np.argsort(ratio, axis=None)[::-1][:count]
    rows = []
    for flat in order:
        idx = np.unravel_index(flat, err.shape)
        rows.append(tuple(int(i) for i in idx) + (float(err[idx]), float(nu[idx]), float(b[idx])))
    return rows


def band_label(name, row):
    """A worst_bands row of output `name` as 'level 2, zone 0' (levels and planes from 1, zones from 0, south to north)."""
    idx = row[:-4]
    return "".join("%s %d, " % (t, i + 1) for t, i in zip(trailing_names(name, len(idx) + 2), idx)) + "zone %d" % row[-4]


def describe(name, rows):
    """worst_bands rows of output `name` as text: 'qtend level 2, zone 0 (rows 0-7): error 1.0e-09, nu 2.2e-16, bound 1.0e-13'
    (levels and planes counted from 1 as the reference does, zones and rows from 0, south to north)."""
    lines = []
    for row in rows:
        idx, (zone, e, v, b) = row[:-4], row[-4:]
        where = "".join(" %s %d," % (t, i + 1) for t, i in zip(trailing_names(name, len(idx) + 2), idx))
        lines.append("%s%s zone %d (rows %d-%d): error %.3e, nu %.3e, bound %.3e" % (
            name, where, zone, zone * ROWS, zone * ROWS + ROWS - 1, e, v, b))
    return "\n".join(lines)


def verdict(got, case, names=None):
    """got: name -> array in host layout (at least the compared part).  -> (failure texts, rows): rows holds per output
    (name, worst error / bound, its band (band_label), whole-field figure)."""
    failures, rows = [], []
    for n in names or case["nu"]:
        g, r = compared(n, got[n]), compared(n, case["ref"][n])
        err = band_errors(g, r)
        worst = worst_bands(err, case["nu"][n])
        over = ~(err <= bound(case["nu"][n]))
        if over.any():
            failures.append("%s, %s: %d of %d bands over the bound; the worst:\n%s" % (
                case["name"], n, int(over.sum()), err.size, describe(n, worst)))
        rows.append((n, worst[0][-3] / worst[0][-1], band_label(n, worst[0]), whole_field(g, r)))
    return failures, rows


def flipped_tops(got, case, member):
    """[(case, member, top, lon, lat)] of the columns whose integer top differs from the oracle's."""
    out = []
    for n in tops(case["shortwave"]):
        out += [(case["name"], member, n, int(lon), int(lat)) for lon, lat in np.argwhere(np.asarray(got[n]) != case["ref"][n])]
    return out


def regime_census(ref, inputs):
    """Counts of columns per regime of one member-step: name -> count, and for the integer tops name -> {value: count}."""
    census = {"precnv > 0": int((ref["precnv"] > 0).sum()), "precls > 0": int((ref["precls"] > 0).sum())}
    for n in TOPS:
        if n in ref:
            values, counts = np.unique(ref[n], return_counts=True)
            census[n] = {int(v): int(c) for v, c in zip(values, counts)}
    if "flux_solar_in" in inputs:
        census["dark"] = int((np.asarray(inputs["flux_solar_in"]) == 0).sum())
    f = np.asarray(inputs["fmask_land"])
    census["sea"], census["land"] = int((f == 0).sum()), int((f == 1).sum())
    census["mixed"] = int(f.size) - census["sea"] - census["land"]
    census["snow"] = int((np.asarray(inputs["snowc"]) > 0).sum())
    return census


def add_census(total, census):
    """Sum `census` into `total` (both as regime_census returns them)."""
    for k, v in census.items():
        if isinstance(v, dict):
            t = total.setdefault(k, {})
            for value, c in v.items():
                t[value] = t.get(value, 0) + c
        else:
            total[k] = total.get(k, 0) + v
    return total


def census_text(census):
    parts = []
    for k, v in census.items():
        parts.append("%s %s" % (k, " ".join("%d:%d" % kv for kv in sorted(v.items())) if isinstance(v, dict) else "%d" % v))
    return ", ".join(parts)


# ---- the cases --------------------------------------------------------------------------------------------------------------
SYNTHETIC_SEEDS = (1, 2, 3)
EDGE_SEED = 4
CO2_SYNTHETIC = 0.3


def zero_tendencies(member):
    out = dict(member)
    for n in TENDENCIES:
        out[n] = np.zeros((96, 48, 8), order="F")
    return out


def edge_member(seed=EDGE_SEED):
    """A synthetic member with the edges the random ones never hit: polar night (flux_solar_in and both ozone fluxes exactly 0)
    in the two southern zones, fmask_land exactly 0 on 45 % and exactly 1 on 45 % of the points and fractional on the rest, and
    no snow at all (snowc exactly 0) on half of the land."""
    from physics_helpers import synthetic_member
    m = synthetic_member(seed=seed)
    rng = np.random.default_rng(1000 + seed)
    pick = rng.uniform(0.0, 1.0, (96, 48))
    fmask = np.where(pick < 0.45, 0.0, np.where(pick < 0.9, 1.0, rng.uniform(0.05, 0.95, (96, 48))))
    m["fmask_land"] = fmask
    m["phis0"] = rng.uniform(0.0, 3000.0, (96, 48)) * (fmask > 0)
    m["snowc"] = np.where((fmask > 0) & (rng.uniform(0.0, 1.0, (96, 48)) < 0.5), 0.0, m["snowc"])
    for n in SOLAR_IN:
        m[n] = m[n].copy()
        m[n][:, :2 * ROWS] = 0.0
    return {k: np.asfortranarray(v, dtype=np.float64) for k, v in m.items()}


def oracle_inputs(member, persisted=None):
    """A member in the layout of physics_helpers.synthetic_member -> the oracle's argument names, tendencies zeroed."""
    out = {("qg_in" if k == "qg" else k): v for k, v in zero_tendencies(member).items()}
    out.update(persisted or {})
    return out


def make_case(oracle, name, inputs, shortwave, co2, draws=DRAWS):
    """inputs: the oracle's arguments (oracle_inputs).  -> the case: name, inputs, shortwave, co2, ref, nu (compared outputs only),
    flipped, census."""
    ref, nu, flipped = noise_floor(lambda x: oracle.physics(x, shortwave, co2), inputs, draws)
    names = outputs(oracle, shortwave)
    ref = {n: a for n, a in ref.items() if n in names or n in tops(shortwave)}
    return dict(name=name, inputs=inputs, shortwave=bool(shortwave), co2=co2, ref=ref, nu={n: nu[n] for n in names},
                flipped=flipped, census=regime_census(ref, inputs))


def persisted_after_shortwave(oracle, inputs, co2):
    """The persisted radiation state that a shortwave step on the same inputs leaves."""
    prev = oracle.physics(inputs, True, co2)
    return {k: prev[k] for k in oracle.PHYS_PERSIST_SHAPES}


def snapshot_member(golden_dir, name):
    """-> (member in synthetic_member's layout with the snapshot's state, persisted state or None, shortwave, co2)."""
    from test_physics_oracle import load_snapshot
    inp, pre, _, sw, co2 = load_snapshot(golden_dir, name)
    inp = {("qg" if k == "qg_in" else k): v for k, v in inp.items()}
    return inp, (None if sw else pre), bool(sw), co2


CASE_NAMES = (("physics_sw", "physics_nosw") + tuple("synthetic%d_%s" % (s, k) for k in ("sw", "nosw") for s in SYNTHETIC_SEEDS)
              + ("edge_sw", "edge_nosw"))
_cases, _members = {}, {}


def member(golden_dir, name):
    """(member, persisted or None) behind a case name; the persisted state of the snapshots only (the synthetic cases' comes
    from the oracle: `case`)."""
    if name not in _members:
        if name.startswith("physics_"):
            _members[name] = snapshot_member(golden_dir, name)[:2]
        else:
            from physics_helpers import synthetic_member
            who = name.split("_")[0]
            key = who + "_"
            if key not in _members:
                _members[key] = (edge_member() if who == "edge" else synthetic_member(seed=int(who[len("synthetic"):])), None)
            _members[name] = _members[key]
    return _members[name]


def case(oracle, golden_dir, name):
    """The case of that name (CASE_NAMES), computed once per session and shared: treat it as read-only."""
    if name not in _cases:
        m, pre = member(golden_dir, name)
        if name.startswith("physics_"):
            _, _, sw, co2 = snapshot_member(golden_dir, name)
        else:
            sw, co2 = name.endswith("_sw"), CO2_SYNTHETIC
            if not sw:
                pre = persisted_after_shortwave(oracle, oracle_inputs(m), co2)
        _cases[name] = make_case(oracle, name, oracle_inputs(m, pre), sw, co2)
    return _cases[name]
