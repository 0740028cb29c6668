"""GPU tier: extremes of the state's grid-space fields over regions and their positions, followed from sample to sample, recorded on
the device (spd_model_tracktape_*, EnsembleModel.tracktape_*).

The arbiter is existing code, the twin of tests/test_projtape_gpu.py: a model built by `perturbed` of tests/test_tape_gpu.py
(t_grid += N(0, 0.01 K), seed = member id) that holds an fp64 TAPE of the names among the entries with every = the recorder's.  The
taped planes are reduced on the CPU by tests/tracktape_reference.py, sample after sample, carrying the follow-state: track, the
numpy restatement that tests/test_tracktape_cpu.py holds to a loop over Python floats and to the library's host compile of the
kernel's routines.  Every comparison is BITWISE, the follow-state after the run included.

A member's trajectory does not depend on how many members its model has or on the launch plan, so one twin of 9 members serves every
fp64 case and one twin of 4 members the fp32-storage case."""
import numpy as np
import pytest

import tracktape_reference as ref
from test_tape_gpu import LEVELS, perturbed

pytestmark = pytest.mark.gpu

EVERY = 3
CALLS = (5, 1, 7, 12, 3, 20)  # 48 steps and 16 samples, most of them inside calls
TOTAL = sum(CALLS)
SAMPLES = TOTAL // EVERY
STATE = ("vor", "div", "t", "tr", "ps")
MIN, MAX = "min", "max"
GLOBE, NATL, DATELINE, COLUMN0, SOUTH, TROPICS, SEAM = range(7)
NATL_BOX = (280.0, 350.0, 30.0, 70.0)  # 80 W ... 10 W, 30 N ... 70 N
Z500 = LEVELS.index(500.0)
# (name, level, region, op, radius); nine entries on the plane of mslp -- three batches of the kernel, the last of one entry --
# under six regions and both ops
ENTRIES = (
    ("mslp", 0, GLOBE, MIN, 0),
    ("mslp", 0, NATL, MIN, 2),       # follows the deepest low of the box from the first sample on
    ("mslp", 0, NATL, MIN, 2),       # FOLLOWED: seeded where the first sample is LARGEST in the box: another low, or none
    ("mslp", 0, NATL, MIN, 0),       # FREE: the same entry, never following
    ("t_grid", 7, GLOBE, MAX, 0),
    ("mslp", 0, DATELINE, MAX, 0),   # a box across the date line
    ("mslp", 0, COLUMN0, MIN, 0),    # the single column i = 0: the western neighbour is column 95
    ("z_plev", Z500, NATL, MIN, 2),
    ("mslp", 0, SOUTH, MAX, 3),      # the southernmost row alone: dj = 0, followed along the row
    ("precnv", 0, TROPICS, MAX, 0),
    ("precnv", 0, TROPICS, MIN, 0),  # TIES at 0.0: the lowest index wins, offsets 0
    ("q_grid", 0, GLOBE, MAX, 0),    # the plane the model holds constant
    ("tcwv", 0, TROPICS, MAX, 4),    # a derived name
    ("t_grid", 7, DATELINE, MIN, 24),
    ("mslp", 0, DATELINE, MIN, 0),   # both ops under one region
    ("precls", 0, GLOBE, MAX, 0),
    ("mslp", 0, SEAM, MIN, 2),       # a box across the seam of the grid at 0 degrees: windows wrap from column 0 to column 95
)
FOLLOWED, FREE, TIES, CONSTANT = 2, 3, 10, 11
NAMES = ("t_grid", "q_grid", "precnv", "precls", "z_plev", "mslp", "tcwv")  # the catalogue's order
ONE = ("precnv", "precls", "mslp", "tcwv")
E = len(ENTRIES)
C_ENTRIES = tuple((n, k, r, {MIN: 0, MAX: 1}[op], rad) for n, k, r, op, rad in ENTRIES)


@pytest.fixture(scope="module")
def bc(golden_dir):
    return np.load(golden_dir + "/../../pyspeedy_amd/data/example_bc.npz")


@pytest.fixture(scope="module")
def regions():
    import pyspeedy_amd
    pw = pyspeedy_amd.projection_weights()
    w = np.stack([pw.global_mean(), pw.box(*NATL_BOX), pw.box(150.0, -150.0, -40.0, 25.0), pw.box(0.0, 0.0, -90.0, 90.0),
                  pw.box(0.0, 360.0, -90.0, -85.0), pw.band(-20.0, 20.0), pw.box(350.0, 10.0, 0.0, 90.0)])
    inside = w != 0
    assert inside[GLOBE].all() and inside[COLUMN0].sum() == 48 and inside[COLUMN0][:, 0].all()
    assert inside[SOUTH].sum() == 96 and inside[SOUTH][0].all()
    assert inside[DATELINE][:, 40].any() and inside[DATELINE][:, 48].any() and inside[DATELINE][:, 56].any() and not inside[DATELINE][:, 0].any()
    assert inside[SEAM].any(axis=0).nonzero()[0].tolist() == [0, 1, 2, 94, 95]
    return w


def twin(spectral, bc, M, fp32=False):
    """dict(planes: {(name, level): numpy [M][16][48][96]} from the twin's fp64 tape, rows, state: the spectral state after step 48)"""
    import torch
    model, _ = perturbed(spectral, bc, M, fp32)
    model.tape_configure(NAMES, EVERY, SAMPLES, dtype="float64")
    model.run(TOTAL)
    assert model.tape_info["taken"] == SAMPLES
    wanted = sorted({(n, k) for n, k, _, _, _ in ENTRIES})
    planes = {}
    for name in NAMES:
        x = model.tape(name)
        for n, k in wanted:
            if n == name:
                planes[(n, k)] = (x if n in ONE else x[:, :, k]).cpu().numpy()
        del x
    rows = model._tape_rows().tolist()
    torch.cuda.synchronize()
    state = {n: [model.get(n, i) for i in range(M)] for n in STATE}
    model.close()
    return dict(planes=planes, rows=rows, state=state)


def seeds_of(tw, regions, M, sample=0):
    """[M][E] int32: -1 but for FOLLOWED, which starts at the point of the box where its plane is largest at `sample`"""
    seeds = np.full((M, E), -1, dtype=np.int32)
    name, level, region = ENTRIES[FOLLOWED][:3]
    for m in range(M):
        x = tw["planes"][(name, level)][m, sample]
        seeds[m, FOLLOWED] = int(np.argmax(np.where(regions[region] != 0, x, -np.inf)))
    return seeds


def reduce(tw, regions, M, seeds, start=0, entries=C_ENTRIES):
    """the reference's series of the samples from `start` on, [M][16 - start][E][4], and the follow-state behind the last, [M][E]"""
    out = np.empty((M, SAMPLES - start, len(entries), 4))
    last = np.empty((M, len(entries)), dtype=np.int32)
    for e, (name, level, region, op, radius) in enumerate(entries):
        for m in range(M):
            out[m, :, e], last[m, e] = ref.follow(tw["planes"][(name, level)][m, start:], regions[region], radius, op, int(seeds[m, e]))
    return out, last


@pytest.fixture(scope="module")
def twin9(spectral, bc):
    return twin(spectral, bc, 9)


def assert_bitwise(got, expected, what):
    """got: a device tensor or numpy, expected: numpy; the bit patterns, so that NaN and the sign of a zero count"""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == expected.shape and got.dtype == expected.dtype, (what, got.shape, expected.shape, got.dtype)
    a, b = got.view(np.uint64), expected.view(np.uint64)
    if not np.array_equal(a, b):
        where = np.argwhere(a != b)[0]
        raise AssertionError("%s: %d of %d values differ, first at %s (entry %s): %r against %r" % (
            what, int((a != b).sum()), a.size, where.tolist(), ENTRIES[where[2]] if got.ndim == 4 else "?", got[tuple(where)],
            expected[tuple(where)]))


def test_the_arbiter_is_not_empty(twin9, regions):
    """On the reference alone: per entry the winner's index varies over the samples and over the members -- but for the entry on the
    plane the model holds constant and the entry whose candidates tie at 0.0, which are asserted to be exactly that; some offset
    lies strictly inside (-0.5, 0.5) and is not zero; and FOLLOWED, seeded at the point of the box where the first sample is
    largest, gives another track than FREE, the same entry with radius 0 -- a recorder that ignored seeds and windows would otherwise
    pass."""
    M = 9
    seeds = seeds_of(twin9, regions, M)
    out, last = reduce(twin9, regions, M, seeds)
    assert out.shape == (M, SAMPLES, E, 4) and np.isfinite(out).all() and (out[..., 1] >= 0).all()
    assert np.array_equal(last, out[:, -1, :, 1].astype(np.int32))
    flat = []
    for e, entry in enumerate(ENTRIES):
        p = out[:, :, e, 1]
        over_samples, over_members = bool((p[:, 1:] != p[:, :-1]).any()), bool((p[1:] != p[:-1]).any())
        inner = int(((out[:, :, e, 2:] != 0) & (np.abs(out[:, :, e, 2:]) < 0.5)).sum())
        print("%-7s level %d region %d %s radius %2d: %3d distinct winners, over samples %d, over members %d, %3d offsets inside" % (
            entry + (len(np.unique(p)), over_samples, over_members, inner)))
        if not (over_samples and over_members):
            flat.append(e)
    assert flat == [TIES, CONSTANT], flat
    # the tie entries really tie: every candidate of the constant plane, and at least two points of the band at the winning 0.0
    name, level, region = ENTRIES[CONSTANT][:3]
    x = twin9["planes"][(name, level)]
    assert (x == x.flat[0]).all() and (out[:, :, CONSTANT, 1] == 0.0).all() and (out[:, :, CONSTANT, 2:] == 0.0).all()
    band = regions[TROPICS] != 0
    dry = twin9["planes"][("precnv", 0)][:, :, band]
    assert (dry.min(axis=2) == 0.0).all() and ((dry == 0.0).sum(axis=2) >= 2).all()
    assert (out[:, :, TIES, 0] == 0.0).all() and (out[:, :, TIES, 2:] == 0.0).all()
    first_dry = np.array([[int(np.flatnonzero(band.ravel() & (twin9["planes"][("precnv", 0)][m, s].ravel() == 0.0))[0]) for s in range(SAMPLES)]
                          for m in range(M)])
    assert np.array_equal(out[:, :, TIES, 1], first_dry)
    offsets = out[..., 2:]
    assert ((offsets != 0) & (np.abs(offsets) < 0.5)).any() and (np.abs(offsets) <= 0.5).all()
    # the followed entry: seeded away from the deepest low, it is somewhere else at one sample at least
    apart = out[:, :, FOLLOWED, 1] != out[:, :, FREE, 1]
    print("FOLLOWED differs from FREE at %d of %d samples; seeds %s" % (int(apart.sum()), apart.size, seeds[:, FOLLOWED].tolist()))
    assert apart.any()
    assert (seeds[:, FOLLOWED] != out[:, 0, FREE, 1]).all()


PLANS = {
    "serial_5": dict(M=5),
    "two_groups_5": dict(M=5, options=(("member_groups", 2),)),
    "rounds_9": dict(M=9, options=(("member_groups", 2), ("block_members", 1)), checked=True),
    "fp32_storage_4": dict(M=4, fp32=True),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_series_equal_the_tracked_tape(spectral, bc, regions, twin9, plan):
    """All entries, a sample every 3 steps over calls of 5, 1, 7, 12, 3 and 20 steps: the ring is bitwise the arbiter's, the rows
    are the tape's, the follow-state after the run is the reference's, and the recording model's spectral state after step 48 is
    bitwise the twin's -- serial, with two uneven member groups, in rounds of block_members with checked calls (the last round
    leaves a group empty), and with fp32 physics storage (precnv / precls stored as float)."""
    import torch
    p = PLANS[plan]
    M, options, fp32, checked = p["M"], p.get("options", ()), p.get("fp32", False), p.get("checked", False)
    tw = twin(spectral, bc, M, fp32=True) if fp32 else twin9
    seeds = seeds_of(tw, regions, M)
    expected, last = reduce(tw, regions, M, seeds)
    model, _ = perturbed(spectral, bc, M, fp32, options)
    model.tracktape_configure(regions, ENTRIES, EVERY, SAMPLES)
    assert (model.tracktape_positions() == -1).all()
    model.tracktape_seed(seeds)
    cfg = model.config()
    if plan == "serial_5":
        assert cfg["chunks"] == 1 and cfg["rounds"] == 1
    if plan == "two_groups_5":
        assert cfg["chunks"] == 2 and cfg["rounds"] == 1
    if plan == "rounds_9":
        assert cfg["chunks"] == 2 and cfg["rounds"] == 5
    if plan == "fp32_storage_4":
        assert cfg["physics_storage32"] and model.device_view("precnv").dtype == torch.float32
    assert model.tracktape_entries == C_ENTRIES
    for n in CALLS:
        if checked:
            failed, _ = model.run_checked(n)
            assert (failed == -1).all()
        else:
            model.run(n)
    assert model.current_step == TOTAL
    assert model.tracktape_info == dict(taken=SAMPLES, held=SAMPLES, capacity=SAMPLES, every=EVERY, regions=len(regions), entries=E)
    assert model._tracktape_rows().tolist() == tw["rows"]
    got = model.tracktape()
    assert got.dtype == torch.float64 and got.is_contiguous() and got.device == model.device_view("t_grid").device
    assert_bitwise(got, expected, plan)
    assert np.array_equal(model.tracktape_positions(), last), plan
    for n, per_member in tw["state"].items():
        for i in range(M):
            assert np.array_equal(model.get(n, i), per_member[i]), (plan, n, i)
    model.close()


def test_ring_reset_seed_and_positions(spectral, bc, regions, twin9):
    """A ring of 5 slots keeps the last five samples with their rows; tracktape_reset empties the ring and un-seeds; a seed comes
    back from tracktape_positions and is refused outside its entry's region or the grid; sub-ranges of members and samples;
    reconfiguring the pressure levels is refused while a pressure-level entry exists; off, calls fail with their reason."""
    import torch
    from pyspeedy_amd._lib import SpeedyHipError
    M = 3
    model, _ = perturbed(spectral, bc, M)
    with pytest.raises(SpeedyHipError, match="no track tape configured"):
        model.tracktape()
    with pytest.raises(SpeedyHipError, match="no track tape configured"):
        model.tracktape_info
    assert model.tracktape_entries == ()
    model.tracktape_configure(regions, ENTRIES, EVERY, 5)
    seeds = seeds_of(twin9, regions, M)
    model.tracktape_seed(seeds)
    assert np.array_equal(model.tracktape_positions(), seeds)
    assert np.array_equal(model.tracktape_positions(first=1, count=2), seeds[1:3])
    for n in CALLS[:3]:  # to step 13: samples at 3, 6, 9, 12
        model.run(n)
    expected, _ = reduce(twin9, regions, M, seeds)
    assert model.tracktape_steps().tolist() == [3, 6, 9, 12] and model.tracktape_info["held"] == 4
    assert_bitwise(model.tracktape(), expected[:, :4], "four samples in five slots")
    model.tracktape_reset()  # at step 13: the ring is empty and nothing is followed
    assert model.tracktape_info == dict(taken=0, held=0, capacity=5, every=EVERY, regions=len(regions), entries=E)
    assert model.tracktape().shape == (M, 0, E, 4) and model.tracktape_steps().tolist() == []
    assert (model.tracktape_positions() == -1).all()
    # a seed round-trips for a part of the members; outside the region, or the grid, it is refused and nothing is written
    some = np.full((2, E), -1, dtype=np.int32)
    some[0, 1], some[1, FOLLOWED], some[1, 6] = seeds[0, FOLLOWED], seeds[2, FOLLOWED], 96 * 47
    model.tracktape_seed(some, first=1)
    assert (model.tracktape_positions(count=1) == -1).all() and np.array_equal(model.tracktape_positions(first=1), some)
    outside = some.copy()
    outside[1, 6] = 96 * 47 + 1  # (row 47, column 1: not in the column i = 0)
    with pytest.raises(SpeedyHipError, match=r"the seed of member 2, entry 6 \(point 4513: row 47, column 1\) lies outside region 3"):
        model.tracktape_seed(outside, first=1)
    for bad in (4608, -2):
        outside[1, 6] = bad
        with pytest.raises(SpeedyHipError, match=r"the seed of member 2, entry 6 \(%d\) is not -1 or 0 ... 4607" % bad):
            model.tracktape_seed(outside, first=1)
    with pytest.raises(SpeedyHipError, match="member range out of bounds"):
        model.tracktape_seed(some, first=2)
    with pytest.raises(ValueError, match="positions must be"):
        model.tracktape_seed(some[:, :3])
    assert np.array_equal(model.tracktape_positions(first=1), some)
    # from sample 4 on with FOLLOWED seeded anew, where ITS plane is largest at sample 4: twelve samples into five slots
    again = seeds_of(twin9, regions, M, sample=4)
    model.tracktape_seed(again)
    model.run(TOTAL - sum(CALLS[:3]))  # one call of 35 steps
    assert model.current_step == TOTAL
    expected, last = reduce(twin9, regions, M, again, start=4)
    assert model.tracktape_info == dict(taken=12, held=5, capacity=5, every=EVERY, regions=len(regions), entries=E)
    assert model._tracktape_rows().tolist() == twin9["rows"][-5:]
    assert model.tracktape_steps().tolist() == [36, 39, 42, 45, 48]
    assert_bitwise(model.tracktape(), expected[:, -5:], "the last five of twelve")
    assert_bitwise(model.tracktape(first=1, count=2, t0=1, nt=3), expected[1:3, -4:-1], "members 1, 2 and samples 1 ... 3")
    assert np.array_equal(model.tracktape_positions(), last)
    buf = torch.empty(4, dtype=torch.float64, device=model.sp.device)
    assert model._lib.spd_model_tracktape_read(model._m, 0, M, 0, 5, buf.data_ptr(), 32, None) == -3  # SPD_E_SIZE
    with pytest.raises(SpeedyHipError, match="sample range out of bounds"):
        model.tracktape(t0=3, nt=3)
    with pytest.raises(SpeedyHipError, match="the track tape holds a pressure-level variable"):
        model.plev_configure([500.0])
    # spd_model_init: an empty ring that follows nothing, the configuration stays
    model.init((1982, 1, 1, 0, 0))
    assert model.tracktape_info["taken"] == 0 and (model.tracktape_positions() == -1).all() and model.tracktape_entries == C_ENTRIES
    model.tracktape_off()
    assert model.tracktape_entries == ()
    for call in (model.tracktape, model.tracktape_reset, model.tracktape_steps, model.tracktape_positions, lambda: model.tracktape_info):
        with pytest.raises(SpeedyHipError, match="no track tape configured"):
            call()
    model.plev_configure([500.0])
    model.run(3)
    model.close()


def test_beside_a_tape_and_a_projection_tape(spectral, bc, regions):
    """Track tape, tape and projection tape on in ONE call of 13 steps with two member groups: the spectral state and both other
    rings are bit for bit those of a run without the track tape, and the track tape's ring and follow-state are those of its solo
    run."""
    import torch
    M, steps = 5, 13
    fields = ("precnv", "mslp")
    proj = (("mslp", 0, NATL), ("precnv", 0, TROPICS), ("t_grid", 7, GLOBE))

    def run(track, others):
        model, _ = perturbed(spectral, bc, M, options=(("member_groups", 2),))
        if others:
            model.tape_configure(fields, 3, 4, dtype="float64")
            model.projtape_configure(regions, proj, 2, 6)
        if track:
            model.tracktape_configure(regions, ENTRIES, 3, 4)
        model.run(steps)
        out = dict(state={n: [model.get(n, i) for i in range(M)] for n in STATE})
        if others:
            out["tape"] = {n: model.tape(n) for n in fields}
            out["tape_steps"] = model.tape_steps().tolist()
            out["proj"] = model.projtape()
        if track:
            out["track"], out["last"], out["steps"] = model.tracktape(), model.tracktape_positions(), model.tracktape_steps().tolist()
        torch.cuda.synchronize()
        model.close()
        return out

    together, without, solo = run(True, True), run(False, True), run(True, False)
    for n in STATE:
        for i in range(M):
            assert np.array_equal(together["state"][n][i], without["state"][n][i]), (n, i)
    for n in fields:
        assert torch.equal(together["tape"][n], without["tape"][n]), n
    assert together["tape_steps"] == without["tape_steps"] == [3, 6, 9, 12]
    assert torch.equal(together["proj"], without["proj"]) and together["proj"].shape == (M, 6, 3)
    assert together["steps"] == solo["steps"] == [3, 6, 9, 12]
    assert_bitwise(together["track"], solo["track"].cpu().numpy(), "beside the others")
    assert np.array_equal(together["last"], solo["last"])
    # ... and what the track tape holds of mslp is the reference's reduction of what the tape beside it holds
    mslp = together["tape"]["mslp"].cpu().numpy()
    for e in (0, 3, 5, 6):
        name, level, region, op, radius = C_ENTRIES[e]
        for m in range(M):
            want, _ = ref.follow(mslp[m], regions[region], radius, op)
            assert_bitwise(together["track"][m, :, e].cpu().numpy(), want, "entry %d of member %d against the tape beside it" % (e, m))
