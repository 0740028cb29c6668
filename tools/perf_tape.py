"""Cost of the tape (time series recorded on the device), 64 members:
(1) ms per model step in 36-step calls without any sampling, with mean-only statistics and with an fp32 tape on the same names and
    `every` (z_plev at 500 hPa alone; all six pressure-level names at 8 levels; every 9 and every 36).  Both run the same front end;
    the tape's store moves 12 bytes per point where the statistics' update moves 24.
(2) the same six-hourly series of z_plev at 500 hPa recorded today's way -- calls of 9 steps, each followed by plev() and a
    device-side copy into a preallocated tensor -- against one tape in 36-step calls.  --today-only runs that leg alone with calls
    the parent commit has as well: a copy of this file in a checkout of the parent measures the parent's build (PYSPEEDY_AMD_LIB
    cannot: the binding refuses a library that lacks a declared symbol).
Variants alternated round by round in one session; medians over the rounds and the spread (max - min) are reported.
(3) --kernel-only: the store kernel in the serial plan (one launch for all members, six names at 8 levels, every step) for a
    `rocprofv3 --kernel-trace --stats` run of its own, and the streaming probe's copy shape at the same bytes in the same session.
Usage: perf_tape.py [--members 64] [--rounds 7] [--calls 4] [--quick] [--today-only] [--kernel-only]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyspeedy_amd  # noqa: E402
from pyspeedy_amd.model import EnsembleModel  # noqa: E402
from pyspeedy_amd.stream_probe import probe  # noqa: E402

LEVELS8 = [925.0, 850.0, 700.0, 500.0, 300.0, 200.0, 100.0, 30.0]
SIX = EnsembleModel.PLEV_VARIABLES
SETS = (("z_plev at 500 hPa", ("z_plev",), [500.0]), ("six names at 8 levels", SIX, LEVELS8))

ap = argparse.ArgumentParser()
ap.add_argument("--members", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=4, help="36-step calls per timing")
ap.add_argument("--quick", action="store_true")
ap.add_argument("--today-only", action="store_true", help="leg (2) without the tape: runs on builds that do not have it")
ap.add_argument("--kernel-only", action="store_true", help="part (3) only: for a kernel trace")
args = ap.parse_args()
rounds = 1 if args.quick else args.rounds
M = args.members

sp = pyspeedy_amd.ModSpectral()
bc = np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))
m = EnsembleModel(sp, M)
m.init_sst_anom(24)
m.set_bc(bc)
m.set_option("prepare_multi_step", 1)
m.run(36)
torch.cuda.synchronize()
start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
steps = 36 * args.calls


def timed(issue):
    torch.cuda.synchronize()
    start.record()
    issue()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def report(title, names, times, base):
    print(title)
    for name in names:
        t = float(np.median(times[name]))
        print("  %-46s %.4f ms per step (max - min %.4f)  %+6.2f %%" % (name, t, max(times[name]) - min(times[name]), 100.0 * (t / base - 1.0)),
              flush=True)


if args.kernel_only:
    m.set_option("member_groups", 1)
    m.plev_configure(LEVELS8)
    m.tape_configure(SIX, 1, 4)
    m.run(36)
    torch.cuda.synchronize()
    planes = 5 * len(LEVELS8) + 1
    nbytes = planes * M * 4608 * 12
    print("store kernel, serial plan, %d members, six names at %d levels: %d planes, %.1f MB per launch (8 B read, 4 B written per point)" % (
        M, len(LEVELS8), planes, nbytes / 1e6))
    for lane_bytes, waves, rows, fl in ((16, 8, 1, 1), (8, 8, 1, 1)):
        tb = [probe(m._lib, sp._h, 1, 1, nbytes, lane_bytes, fl, 1, waves, rows, 10, 0)["tb_s"] for _ in range(rounds + 1)][1:]
        print("  streaming probe 1r:1w at the same bytes, %d B per lane, non-temporal: %.2f TB/s (max - min %.2f)  = %.1f us" % (
            lane_bytes, float(np.median(tb)), max(tb) - min(tb), nbytes / float(np.median(tb)) / 1e6), flush=True)
    m.close()
    sys.exit(0)

# ---- (2) today's way: calls of 9 steps, plev() and a device-side copy after each ----
m.plev_configure([500.0])
series = torch.empty((M, steps // 9, 1, 48, 96), dtype=torch.float32, device=sp.device)


def todays_way():
    for k in range(steps // 9):
        m.run(9)
        series[:, k].copy_(m.plev(["z_plev"])["z_plev"])


def with_tape():
    for _ in range(args.calls):
        m.run(36)


legs = {"calls of 9 steps + plev() + copy (today's way)": []}
if not args.today_only:
    legs["one tape (fp32, every 9) in 36-step calls"] = []
    legs["no output, 36-step calls"] = []
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for name in legs:
        if name.startswith("calls of 9"):
            t = timed(todays_way)
        else:
            m.tape_configure(("z_plev",) if name.startswith("one tape") else [], 9, steps // 9)
            m.run(36)
            t = timed(with_tape)
            m.tape_configure([], 1, 1)
        if r > 0:
            legs[name].append(t)
base = float(np.median(legs[list(legs)[-1]]))
report("%d members, z_plev at 500 hPa every 9 steps over %d steps per timing, %d rounds%s" % (
    M, steps, rounds, " (--today-only)" if args.today_only else ""), list(legs), legs, base)
if args.today_only:
    m.close()
    sys.exit(0)

# ---- (1) the cost of a sample: statistics (mean only) against the tape (fp32) ----
VARIANTS = [("none", None, None, None, None)]
for every in (9, 36):
    for label, names, levels in SETS:
        VARIANTS.append(("statistics, %s, every %d" % (label, every), "stats", names, levels, every))
        VARIANTS.append(("tape, %s, every %d" % (label, every), "tape", names, levels, every))
times = {v[0]: [] for v in VARIANTS}
for r in range(rounds + 1):
    for name, kind, names, levels, every in VARIANTS:
        m.stats_configure([], 1)
        m.tape_configure([], 1, 1)
        if levels:
            m.plev_configure(levels)
        if kind == "stats":
            m.stats_configure(names, every, False)
        elif kind == "tape":
            m.tape_configure(names, every, 4)
        m.run(36)
        t = timed(with_tape)
        if r > 0:
            times[name].append(t)
report("%d members, %d calls of 36 steps per timing, %d rounds; statistics mean only, tape fp32 with 4 slots; groups: %d" % (
    M, args.calls, rounds, m.config()["chunks"]), [v[0] for v in VARIANTS], times, float(np.median(times["none"])))
m.close()
