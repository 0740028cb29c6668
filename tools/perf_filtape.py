"""Cost of the filter tape (window means and covariances of time-filtered fields, filtered and accumulated behind the sampled
steps), 64 members, default plan: ms per model step in 36-step calls
    off                   no recorder
    tape (yardstick)      an fp32 tape of the same names (z_plev, u_plev, v_plev, t_plev at 850, 500 and 250 hPa), a sample every 9
                          steps: the same front end plus a store
    filter tape, filters  examples/bandpass_storm_tracks.py's configuration with a spin-up longer than the run: the front end and the
                          filter launch, no accumulate launch
    filter tape           the same configuration counting every sample: both launches on every sampled step, monthly windows
The recorder's own cost is what lies above the yardstick; the accumulate launch is what the last line adds to the one before it.
Variants alternated round by round in one session; medians over the rounds and the spread (max - min) are reported, and the
traffic the two launches move by the recorder's own layout.  The two kernels' own times come from a run of this tool with --quick
under a kernel trace.
Usage: perf_filtape.py [--members 64] [--rounds 7] [--calls 4] [--sample-every 9] [--quick]"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyspeedy_amd  # noqa: E402
from pyspeedy_amd.model import EnsembleModel  # noqa: E402

spec = importlib.util.spec_from_file_location("bandpass_storm_tracks", os.path.join(ROOT, "examples", "bandpass_storm_tracks.py"))
example = importlib.util.module_from_spec(spec)
spec.loader.exec_module(example)

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
m.plev_configure([850.0, 500.0, 250.0])
m.run(36)
torch.cuda.synchronize()
steps = 36 * args.calls
start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
FILTERS, ENTRIES = example.filters(), example.entries()
NAMES = ["z_plev", "u_plev", "v_plev", "t_plev"]


def timed():
    torch.cuda.synchronize()
    start.record()
    for _ in range(args.calls):
        m.run(36)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def all_off():
    m.tape_configure([], 1, 1)
    if m.filtape_entries:
        m.filtape_off()


VARIANTS = ("off", "tape (yardstick)", "filter tape, filters", "filter tape")
times = {v: [] for v in VARIANTS}
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for name in VARIANTS:
        all_off()
        if name == "tape (yardstick)":
            m.tape_configure(NAMES, args.sample_every, 8)
        elif name == "filter tape, filters":
            m.filtape_configure(FILTERS, ENTRIES, "month", 4, sample_every=args.sample_every, spinup=10 ** 9)
        elif name == "filter tape":
            m.filtape_configure(FILTERS, ENTRIES, "month", 4, sample_every=args.sample_every, spinup=0)
        m.run(36)
        t = timed()
        if r > 0:
            times[name].append(t)
all_off()
base, yard = float(np.median(times["off"])), float(np.median(times["tape (yardstick)"]))
print("%d members, groups: %d, a sample every %d steps, monthly windows, %d calls of 36 steps per timing, %d rounds; fp32 ring" % (
    M, m.config()["chunks"], args.sample_every, args.calls, rounds))
for name in VARIANTS:
    t = float(np.median(times[name]))
    print("  %-21s %.4f ms per step (max - min %.4f)  %+6.2f %% over off  %+.4f ms per step, %+.4f ms per sampled step over the yardstick"
          "  all rounds: %s" % (name, t, max(times[name]) - min(times[name]), 100.0 * (t / base - 1.0), t - yard, (t - yard) * args.sample_every,
                                " ".join("%.4f" % v for v in times[name])), flush=True)
# the traffic of one sampled step by the layout: per filtered plane x in, the state of its sections in and out, y out; per entry
# y_a and y_b in (a variance reads one) and the accumulator in and out
plane = 4608 * 8
sections = {0: len(FILTERS[0]), 1: len(FILTERS[1])}
filtered = {(e[0], e[1], e[2]) for e in ENTRIES} | {(e[4], e[5], e[2]) for e in ENTRIES if len(e) == 6}
filter_bytes = sum(plane * (1 + 4 * sections[f] + 1) for _, _, f in filtered) * M
acc_bytes = sum(plane * ((2 if len(e) == 6 else 1) + 2) for e in ENTRIES) * M
print("  %d filtered planes, %d entries: the filter launch moves %.1f MB per sampled step, the accumulate launch %.1f MB "
      "(reads of y and read and write of the accumulators; a close adds %.1f MB of ring stores)" % (
          len(filtered), len(ENTRIES), filter_bytes / 1e6, acc_bytes / 1e6, len(ENTRIES) * 4608 * 4 * M / 1e6))
m.close()
