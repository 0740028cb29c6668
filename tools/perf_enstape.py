"""Cost of the ensemble tape (mean and spread over the members recorded on the device), 64 members, default plan, names z_plev at
500 hPa and mslp, every 9 steps:
(1) ms per model step in 36-step calls with the ensemble tape, with an fp32 tape of the same names and `every`, and with neither.
    Both recorders run the same front end and read the same slab; the tape's store writes M planes per name and sample, the fold
    two per member group.  The tape is measured in the same session on the same build: it is the yardstick.
    Variants alternated round by round in one session; medians over the rounds and the spread (max - min) are reported.
(2) --kernel-only: the ensemble tape on every step for a `rocprofv3 --kernel-trace --stats` run of its own (the fold kernel's mean
    launch time; one launch per member group and sample).
Usage: perf_enstape.py [--members 64] [--rounds 7] [--calls 4] [--every 9] [--quick] [--kernel-only]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyspeedy_amd  # noqa: E402
from pyspeedy_amd.model import EnsembleModel  # noqa: E402

NAMES = ("z_plev", "mslp")

ap = argparse.ArgumentParser()
ap.add_argument("--members", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=4, help="36-step calls per timing")
ap.add_argument("--every", type=int, default=9)
ap.add_argument("--quick", action="store_true")
ap.add_argument("--kernel-only", action="store_true", help="part (2) only: for a kernel trace")
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

if args.kernel_only:
    m.enstape_configure(NAMES, 1, 36)  # (a ring as long as a call: a sample the same call would overwrite is not folded at all)
    for _ in range(args.calls):
        m.run(36)
    torch.cuda.synchronize()
    cfg = m.config()
    print("fold kernel: %d members in %d groups, %d planes, every step of %d: %d launches of enstape_fold_kernel, each reading %.2f MB" % (
        M, cfg["chunks"], len(NAMES), steps, cfg["chunks"] * steps, len(NAMES) * 4608 * 8 * (M / cfg["chunks"]) / 1e6))
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


VARIANTS = ("neither", "tape, fp32", "ensemble tape")
times = {v: [] for v in VARIANTS}
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for name in VARIANTS:
        m.tape_configure([], 1, 1)
        m.enstape_configure([], 1, 1)
        if name.startswith("tape"):
            m.tape_configure(NAMES, args.every, 4, dtype="float32")
        elif name.startswith("ensemble"):
            m.enstape_configure(NAMES, args.every, 4)
        m.run(36)
        t = timed()
        if r > 0:
            times[name].append(t)
base = float(np.median(times["neither"]))
print("%d members, groups: %d, %s every %d steps, %d calls of 36 steps per timing, %d rounds; both rings with 4 slots" % (
    M, m.config()["chunks"], " + ".join(NAMES), args.every, args.calls, rounds))
for name in VARIANTS:
    t = float(np.median(times[name]))
    print("  %-16s %.4f ms per step (max - min %.4f)  %+6.2f %%  all rounds: %s" % (
        name, t, max(times[name]) - min(times[name]), 100.0 * (t / base - 1.0), " ".join("%.4f" % v for v in times[name])), flush=True)
m.close()
