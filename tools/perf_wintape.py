"""Cost of the window tape (window means, extremes and threshold counts of the state's fields, accumulated behind the sampled
steps), 64 members, default plan: ms per model step in 36-step calls
    off                 no recorder
    tape (yardstick)    an fp32 tape of z_plev at 500 hPa and mslp, a sample every 9 steps: the same front end plus a store
    window tape, small  the monthly mean of the same two names, a sample every 9 steps
    window tape, full   examples/monthly_climate.py's configuration (z_plev and mslp mean, wspd_grid max, t_grid min, max and
                        count below 273.15 K), a sample every 9 steps, monthly windows
The recorder's own cost is what lies above the yardstick.  Variants alternated round by round in one session; medians over the
rounds and the spread (max - min) are reported.
Usage: perf_wintape.py [--members 64] [--rounds 7] [--calls 4] [--sample-every 9] [--quick]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyspeedy_amd  # noqa: E402
from pyspeedy_amd.model import EnsembleModel  # noqa: E402

SMALL = (("z_plev", "mean"), ("mslp", "mean"))
FULL = (("z_plev", "mean"), ("mslp", "mean"), ("wspd_grid", "max"), ("t_grid", "min"), ("t_grid", "max"),
        ("t_grid", "count_below", 273.15))

ap = argparse.ArgumentParser()
ap.add_argument("--members", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=4, help="36-step calls per timing")
ap.add_argument("--sample-every", type=int, default=9)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()
rounds = 1 if args.quick else args.rounds
M = args.members

sp = pyspeedy_amd.ModSpectral()
bc = np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))
m = EnsembleModel(sp, M)
m.init_sst_anom(24)
m.set_bc(bc)
m.set_option("prepare_multi_step", 1)
m.plev_configure([500.0])
m.run(36)
torch.cuda.synchronize()
steps = 36 * args.calls
start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed():
    torch.cuda.synchronize()
    start.record()
    for _ in range(args.calls):
        m.run(36)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


VARIANTS = ("off", "tape (yardstick)", "window tape, small", "window tape, full")
times = {v: [] for v in VARIANTS}
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for name in VARIANTS:
        m.tape_configure([], 1, 1)
        m.wintape_configure([], 1, 1)
        if name == "tape (yardstick)":
            m.tape_configure(["z_plev", "mslp"], args.sample_every, 8)
        elif name == "window tape, small":
            m.wintape_configure(SMALL, "month", 4, sample_every=args.sample_every)
        elif name == "window tape, full":
            m.wintape_configure(FULL, "month", 4, sample_every=args.sample_every)
        m.run(36)
        t = timed()
        if r > 0:
            times[name].append(t)
m.tape_configure([], 1, 1)
m.wintape_configure([], 1, 1)
base, yard = float(np.median(times["off"])), float(np.median(times["tape (yardstick)"]))
print("%d members, groups: %d, a sample every %d steps, monthly windows, %d calls of 36 steps per timing, %d rounds; fp32 rings" % (
    M, m.config()["chunks"], args.sample_every, args.calls, rounds))
for name in VARIANTS:
    t = float(np.median(times[name]))
    print("  %-20s %.4f ms per step (max - min %.4f)  %+6.2f %% over off  %+6.2f %% over the yardstick  all rounds: %s" % (
        name, t, max(times[name]) - min(times[name]), 100.0 * (t / base - 1.0), 100.0 * (t / yard - 1.0),
        " ".join("%.4f" % v for v in times[name])), flush=True)
m.close()
