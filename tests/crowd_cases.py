"""The configuration of the crowd tests (tests/test_crowd_gpu.py) and the schedule of a call restated in Python.

Every in-loop feature is switched on in ONE model and stepped through the same calls as a model that carries that feature alone.
This file holds what both tiers need: the periods, the calls, the launch plans, the entries of every consumer, and -- written from
DESIGN sections 4a - 4o, not from the library's source -- where `spd_model_step` cuts a call and at which steps each consumer is due.

The schedule in words.  A recorder with period e samples after every step that leaves the step counter at a multiple of e; the
accumulation tape and the window tape close a window there (the first window opens at the step of their _configure).  A joined
consumer that loops -- breeding or assimilation, the verification tape, the quantile tape -- cuts the call at the multiples of its
own period; what lies between two cuts (or a cut and an end of the call) is a segment, "a call of its own".  At a cut the events
go out in this order: the quantile sample, the verification's phase 0, the rescale or the analysis, and behind an analysis that was
applied the verification's phase 1.  An analysis is applied only at a step that a row of observations is stamped with.

tests/test_crowd_cpu.py asserts on these numbers the conditions that make the GPU tier about what it claims."""
import numpy as np

START = 30
CALLS = (5, 1, 7, 12, 3, 20)
END = START + sum(CALLS)
SOLO_CALL = 40   # the call of the case without a joined consumer: one segment, long enough for the second group's offset
OFFSET_FROM = 36  # segments shorter than this start both member groups together
EXTRA = 7        # the steps behind every *_off() of the last case

# ---- periods ---------------------------------------------------------------------------------------------------------------------
DRIVER_EVERY, VERIF_EVERY, QTAPE_EVERY = 6, 4, 9
JOINED = {"driver": DRIVER_EVERY, "verif": VERIF_EVERY, "qtape": QTAPE_EVERY}
EVERY = {"stats": 2, "tape": 1, "spectra": 4, "enstape": 5, "acctape": 4, "wintape": 6, "projtape": 2, "verif": VERIF_EVERY,
         "qtape": QTAPE_EVERY, "breed": DRIVER_EVERY, "assim": DRIVER_EVERY}
WIN_SAMPLE_EVERY = 2
# the rings: every one but the tape's (the arbiters read all of its samples) is smaller than the number of its events
CAPACITY = {"tape": END - START, "spectra": 5, "enstape": 4, "acctape": 5, "wintape": 3, "projtape": 5, "verif": 5, "qtape": 3,
            "breed": 3, "assim": 2}
SMALL = tuple(k for k in CAPACITY if k != "tape")
# the steps the assimilation has observations for: the events of 48, 54, 60, 66 and 78 find none.  72 is due for all three joined
# consumers and still held by the small rings at the end: the quantile sample and both phases of the verification stand there
# beside an analysis that was applied
ROWS = (36, 42, 72)

# ---- entries -----------------------------------------------------------------------------------------------------------------------
LEVELS_HPA = (500.0,)
# weight maps: 0 the global mean, 1 a box across the date line, 2 N(0, 1), 3 a station stencil
BOX, STATION, MAP_SEED = (150.0, -150.0, -40.0, 25.0), (39.0, -30.0), 2027
TAPED = ("t_grid", "ps_grid", "precnv", "precls", "z_plev", "mslp", "tcwv")
DERIVE_TAPED, PLEV_TAPED = ("tcwv",), ("z_plev", "mslp")
STATS = ("t_grid", "precnv", "precls", "mslp")
SPECTRA = ("ke_rot_spectrum", "t_spectrum", "lnps_mean")
ENSTAPE = ("ps_grid", "precls", "z_plev", "tcwv")
ACCTAPE = (("precnv", "sum"), ("precls", "max"), ("olr", "mean"), ("ustr", "mean"))
WINTAPE = (("t_grid", "mean"), ("precnv", "max"), ("wspd_grid", "max"), ("mslp", "min"), ("tcwv", "count_above", 20.0))
PROJTAPE = (("t_grid", 0, 0), ("t_grid", 7, 1), ("ps_grid", 0, 0), ("precnv", 0, 0), ("precls", 0, 2), ("mslp", 0, 1), ("z_plev", 0, 0),
            ("tcwv", 0, 0))
VERIF = (("t_grid", 0, 2), ("t_grid", 7, 0), ("ps_grid", 0, 0), ("precnv", 0, 0), ("precls", 0, 1), ("mslp", 0, 1), ("z_plev", 0, 0),
         ("tcwv", 0, 2))
QTAPE = (("t_grid", 0, "min"), ("t_grid", 7, "quantile", 0.5), ("ps_grid", 0, "max"), ("precnv", 0, "prob_above", 0.0),
         ("precnv", 0, "quantile", 0.9), ("precls", 0, "max"), ("mslp", 0, "prob_below", 101325.0), ("z_plev", 0, "quantile", 1.0 / 3.0),
         ("tcwv", 0, "quantile", 0.5))
VERIF_PRECNV, QTAPE_PRECNV, QTAPE_PRECNV_Q = 3, 3, 4
ASSIM = (("t_grid", 7, 3), ("t_grid", 0, 1), ("ps_grid", 0, 0), ("mslp", 0, 1))  # (the assimilation refuses precnv and precls)
INFLATION = 1.05
NUDGE_STAMPS = (20, 150)  # two target times that bracket every step of the test

RECORDERS = ("stats", "tape", "spectra", "enstape", "acctape", "wintape", "projtape", "derive", "plev")  # issued per member group
JOINED_CONSUMERS = ("verif", "qtape")
CONSUMERS = RECORDERS + JOINED_CONSUMERS
# the consumers that can be switched off on their own, in the order the last case does it (the tape first: from then on the
# union in `p.diag` is no longer held at 1 by a precipitation sample on every step)
OFF_ORDER = ("tape", "stats", "spectra", "enstape", "acctape", "wintape", "projtape", "verif", "qtape")

# ---- plans -------------------------------------------------------------------------------------------------------------------------
# control: the breeding's control of every member (driver A); assim: the assimilation's mask (driver B)
PLANS = {
    "serial_5": dict(members=5, options=(), fp32=False, verif=((1, 1, 0, 0, 1), 2), qtape=(1, 0, 1, 1, 1),
                     control=(-1, 0, -1, 0, 2), assim=None),
    "groups_rounds_12": dict(members=12, options=(("member_groups", 2), ("block_members", 2), ("tau_recompute", 2)), fp32=False,
                             verif=((1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 0, 1), 10), qtape=(0, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 0),
                             control=(-1, 0, -1, -1, -1, 0, -1, -1, -1, 7, -1, 7), assim=(1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 1)),
    "fp32_storage_6": dict(members=6, options=(("member_groups", 2),), fp32=True, verif=((1, 0, 1, 1, 0, 1), 4),
                           qtape=(0, 1, 1, 0, 1, 1), control=None, assim=(1, 1, 0, 1, 0, 1)),
}
CASES = (("serial_5", "A"), ("groups_rounds_12", "A"), ("groups_rounds_12", "B"), ("fp32_storage_6", "B"))


def weight_maps():
    import pyspeedy_amd
    pw = pyspeedy_amd.projection_weights()
    return np.stack([pw.global_mean(), pw.box(*BOX), np.random.default_rng(MAP_SEED).normal(0.0, 1.0, (48, 96)), pw.point(*STATION)])


def masked(mask):
    return [i for i, v in enumerate(mask) if v]


# ---- the schedule --------------------------------------------------------------------------------------------------------------------
def due(every, start, stop):
    """the steps n in (start, stop] that a consumer of period `every` is due behind"""
    return [n for n in range(start + 1, stop + 1) if n % every == 0]


def call_segments(c0, nsteps, periods):
    """one call of `nsteps` steps that begins at step counter c0, cut at the multiples of `periods` -> [(c0, length)]"""
    out, end = [], c0 + nsteps
    while c0 < end:
        nxt = min([end] + [(c0 // e + 1) * e for e in periods])
        out.append((c0, nxt - c0))
        c0 = nxt
    return out


def segments(start=START, calls=CALLS, periods=tuple(JOINED.values())):
    out = []
    for n in calls:
        out += call_segments(start, n, periods)
        start += n
    return out


def call_ends(start=START, calls=CALLS):
    return list(np.cumsum(calls) + start)


def events_at(step, driver, rows=ROWS, joined=JOINED):
    """the joined events behind the segment that ends at `step`, in their order; driver "A" (breeding) or "B" (assimilation)"""
    out = []
    if "qtape" in joined and step % joined["qtape"] == 0:
        out.append("qtape")
    scored = "verif" in joined and step % joined["verif"] == 0
    if scored:
        out.append("verif0")
    if "driver" in joined and step % joined["driver"] == 0:
        if driver == "A":
            out.append("rescale")
        else:
            out.append("analysis" if step in rows else "skipped")
            if scored and step in rows:
                out.append("verif1")
    return out


def window_rows(every, start, stop, sample_every=1):
    """the windows of a window recorder configured at `start` that close up to `stop`: [(closing step, samples, steps)], and
    the open one behind them as (its first step's counter before the step, samples so far)"""
    rows, opened = [], start
    for n in due(every, start, stop):
        rows.append((n, len(due(sample_every, opened, n)), n - opened))
        opened = n
    return rows, (opened, len(due(sample_every, opened, stop)))


def ring_steps(name, driver="A", start=START, stop=END):
    """the stamps of every event of one ring between `start` (where it was configured) and `stop`, oldest first"""
    if name == "assim":
        return [n for n in due(EVERY[name], start, stop) if n in ROWS]
    return due(EVERY[name], start, stop)


def held(steps, name):
    return steps[-CAPACITY[name]:]


def wraps(name, driver="A", start=START, stop=END, segs=None):
    """-> (inside, across): the number of times the ring's write position went from its last slot to its first between two
    events of one segment, and between events that a cut or an end of a call separates"""
    segs = segments() if segs is None else segs
    index = {}
    for k, (c0, n) in enumerate(segs):
        for s in range(c0 + 1, c0 + n + 1):
            index[s] = k
    steps, cap = ring_steps(name, driver, start, stop), CAPACITY[name]
    inside = across = 0
    for k in range(cap, len(steps), cap):
        if index[steps[k - 1]] == index[steps[k]]:
            inside += 1
        else:
            across += 1
    return inside, across


def census(segs):
    """the text of a segment list for the record: how many, of which lengths, entered at which phase of the shortwave cycle"""
    lengths = [n for _, n in segs]
    by_len = {n: lengths.count(n) for n in sorted(set(lengths))}
    by_phase = {p: sum(1 for c0, n in segs if c0 % 3 == p and n >= 2) for p in range(3)}
    return "%d segments, lengths %s, of two steps and more by c0 %% 3: %s" % (len(segs), by_len, by_phase)
