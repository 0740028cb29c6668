"""Cost of the spectra (spectra by total wavenumber and global means recorded on the device), 64 members:
(1) ms per model step in 36-step calls without any sampling, and with all eight names recorded every step and every 9 steps.
    Variants alternated round by round in one session; medians over the rounds and the spread (max - min) are reported, and the
    bytes the kernel reads per sample (33 planes of 15 872 B per member) beside them.
(2) --kernel-only: the kernel in the serial plan (one launch for all members, all names, every step) for a
    `rocprofv3 --kernel-trace --stats` run of its own.
Usage: perf_spectra.py [--members 64] [--rounds 7] [--calls 4] [--quick] [--kernel-only]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyspeedy_amd  # noqa: E402
from pyspeedy_amd.model import EnsembleModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--members", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=4, help="36-step calls per timing")
ap.add_argument("--quick", action="store_true")
ap.add_argument("--kernel-only", action="store_true", help="part (2) only: for a kernel trace")
args = ap.parse_args()
rounds = 1 if args.quick else args.rounds
M = args.members
NAMES = EnsembleModel.SPECTRA_NAMES
READ_MB = M * 33 * 15872 / 1e6  # vorticity, divergence, temperature, humidity at 8 levels and ln ps

sp = pyspeedy_amd.ModSpectral()
bc = np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))
m = EnsembleModel(sp, M)
m.init_sst_anom(24)
m.set_bc(bc)
m.set_option("prepare_multi_step", 1)
m.run(36)
torch.cuda.synchronize()

if args.kernel_only:
    m.set_option("member_groups", 1)
    m.spectra_configure(NAMES, 1, 4)
    m.run(36)
    torch.cuda.synchronize()
    print("spectra_kernel, serial plan, %d members, all names: 36 launches of %d workgroups, %.1f MB read per launch" % (M, 9 * M, READ_MB))
    m.close()
    sys.exit(0)

start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
steps = 36 * args.calls


def timed():
    torch.cuda.synchronize()
    start.record()
    for _ in range(args.calls):
        m.run(36)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


VARIANTS = [("none", None), ("all names, every step", 1), ("all names, every 9 steps", 9)]
times = {v[0]: [] for v in VARIANTS}
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for name, every in VARIANTS:
        m.spectra_configure(NAMES if every else [], every or 1, 4)
        m.run(36)
        t = timed()
        if r > 0:
            times[name].append(t)
base = float(np.median(times["none"]))
print("%d members, %d calls of 36 steps per timing, %d rounds; 4 slots; groups: %d; %.1f MB read per sample" % (
    M, args.calls, rounds, m.config()["chunks"], READ_MB))
for name, every in VARIANTS:
    t = float(np.median(times[name]))
    line = "  %-28s %.4f ms per step (max - min %.4f)  %+6.2f %%" % (name, t, max(times[name]) - min(times[name]), 100.0 * (t / base - 1.0))
    if every:
        line += "   = %.2f us per sample" % ((t - base) * every * 1e3)
    print(line, flush=True)
m.close()
