"""Cost of the accumulation tape (window sums, means and extremes of the physics fluxes, accumulated behind every step), 64
members, default plan, windows of 36 steps:
(1) ms per model step in 36-step calls with the recorder off, with only set_option("diag_every_step", 1), with the recorder holding
    sum of precnv + precls and mean of olr, and with the recorder holding all names under all ops.  While the recorder is on every
    step stores its diagnostics-only outputs, which is what diag_every_step does on its own: that line is the yardstick, and the
    recorder's own cost is what lies above it.
    Variants alternated round by round in one session; medians over the rounds and the spread (max - min) are reported.
(2) --kernel-only: the small configuration for a `rocprofv3 --kernel-trace --stats` run of its own (the accumulate kernel's mean
    launch time; one launch per member group and step).
Usage: perf_acctape.py [--members 64] [--rounds 7] [--calls 4] [--every 36] [--quick] [--kernel-only] [--all]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyspeedy_amd  # noqa: E402
from pyspeedy_amd.model import EnsembleModel  # noqa: E402

SMALL = (("precnv", "sum"), ("precls", "sum"), ("olr", "mean"))
EVERYTHING = tuple((n, op) for n in EnsembleModel.ACCTAPE_NAMES for op in ("sum", "mean", "min", "max"))

ap = argparse.ArgumentParser()
ap.add_argument("--members", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=4, help="36-step calls per timing")
ap.add_argument("--every", type=int, default=36)
ap.add_argument("--quick", action="store_true")
ap.add_argument("--kernel-only", action="store_true", help="part (2) only: for a kernel trace")
ap.add_argument("--all", action="store_true", help="with --kernel-only: all names and ops instead of the small configuration")
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
steps = 36 * args.calls


def planes(entries):
    """(source planes read per step, accumulators read and written per step)"""
    three = EnsembleModel.ACCTAPE_THREE_PLANES
    src = sum(3 if n in three else 1 for n in {n for n, _ in entries})
    acc = sum(3 if n in three else 1 for n, kind in {(n, "s" if op in ("sum", "mean") else op) for n, op in entries})
    return src, acc


if args.kernel_only:
    entries = EVERYTHING if args.all else SMALL
    m.acctape_configure(entries, args.every, 4)
    for _ in range(args.calls):
        m.run(36)
    torch.cuda.synchronize()
    cfg = m.config()
    src, acc = planes(entries)
    print("accumulate kernel: %d members in %d groups, %d source planes and %d accumulators, %d steps: %d launches of "
          "acctape_step_kernel, a step moving at most %.1f MB (sources fp64)" % (
              M, cfg["chunks"], src, acc, steps, cfg["chunks"] * steps, (src + 2 * acc) * 4608 * 8 * M / 1e6))
    m.close()
    sys.exit(0)

start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed():
    torch.cuda.synchronize()
    start.record()
    for _ in range(args.calls):
        m.run(36)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


VARIANTS = ("off", "diag_every_step", "recorder, small", "recorder, all")
times = {v: [] for v in VARIANTS}
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for name in VARIANTS:
        m.acctape_configure([], 1, 1)
        m.set_option("diag_every_step", 1 if name == "diag_every_step" else 0)
        if name == "recorder, small":
            m.acctape_configure(SMALL, args.every, 4)
        elif name == "recorder, all":
            m.acctape_configure(EVERYTHING, args.every, 4)
        m.run(36)
        t = timed()
        if r > 0:
            times[name].append(t)
m.set_option("diag_every_step", 0)
base, yard = float(np.median(times["off"])), float(np.median(times["diag_every_step"]))
print("%d members, groups: %d, windows of %d steps, %d calls of 36 steps per timing, %d rounds; fp32 rings with 4 slots" % (
    M, m.config()["chunks"], args.every, args.calls, rounds))
print("  small: %s (%d source planes, %d accumulators); all: %d entries (%d source planes, %d accumulators)" % (
    ", ".join("%s of %s" % (op, n) for n, op in SMALL), *planes(SMALL), len(EVERYTHING), *planes(EVERYTHING)))
for name in VARIANTS:
    t = float(np.median(times[name]))
    print("  %-16s %.4f ms per step (max - min %.4f)  %+6.2f %% over off  %+6.2f %% over diag_every_step  all rounds: %s" % (
        name, t, max(times[name]) - min(times[name]), 100.0 * (t / base - 1.0), 100.0 * (t / yard - 1.0),
        " ".join("%.4f" % v for v in times[name])), flush=True)
m.close()
