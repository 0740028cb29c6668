"""Cost of the pressure-level fields on the device, 64 members: (1) the kernel alone (5 variables + mslp at 8 levels, from the grid
arrays) in microseconds and TB/s over its algorithmic bytes, next to what the streaming probe moves in the 2 reads : 1 write shape
at the same size in the same session; (2) ms per model step in 36-step calls without statistics, with t_grid-only statistics, with
z_plev at 500 hPa alone and with all six names at 8 levels, sampled every 9 or 36 steps (mean only).  Variants alternated round by
round in one session; medians over the rounds and the spread (max - min) are reported.
Usage: perf_plev.py [--members 64] [--rounds 7] [--calls 4] [--quick] [--kernel-only]   (--quick: one round; --kernel-only: part (1)
alone, for `rocprofv3 --kernel-trace --stats`)"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyspeedy_amd  # noqa: E402
from pyspeedy_amd import _lib  # noqa: E402
from pyspeedy_amd.model import EnsembleModel  # noqa: E402
from pyspeedy_amd.stream_probe import probe  # noqa: E402

LEVELS8 = [925.0, 850.0, 700.0, 500.0, 300.0, 200.0, 100.0, 30.0]
SIX = EnsembleModel.PLEV_VARIABLES
VARIANTS = [("none", None, None, None)]
for every in (9, 36):
    VARIANTS += [("t_grid, every %d" % every, ("t_grid",), None, every), ("z_plev at 500 hPa, every %d" % every, ("z_plev",), [500.0], every),
                 ("six names at 8 levels, every %d" % every, SIX, LEVELS8, every)]

ap = argparse.ArgumentParser()
ap.add_argument("--members", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=4, help="36-step calls per timing")
ap.add_argument("--quick", action="store_true")
ap.add_argument("--kernel-only", action="store_true", help="part (1) only: for a kernel trace of the kernel alone")
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

# ---- (1) the kernel alone ----
m.plev_configure(LEVELS8)
m.plev()  # (allocates the results, refreshes the grid arrays)
L, stream = m._lib, m._stream()
names = (C.c_char_p * 1)()
planes_in, planes_out = 5 * 8 + 2, 5 * len(LEVELS8) + 1  # + ps, phis0 | + mslp
nbytes = (planes_in + planes_out) * M * 4608 * 8
launches = 20
kernel_us, probe_tb = [], []
h = sp._h
for r in range(rounds + 1):
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        _lib.check(L.spd_model_plev_compute(m._m, names, 0, 0, M, 0, stream), "spd_model_plev_compute")
    stop.record()
    stop.synchronize()
    if r > 0:
        kernel_us.append(1e3 * start.elapsed_time(stop) / launches)
    # the probe in the same session: 2 reads : 1 write, one double per lane, 8 wavefronts per SIMD, short-lived wavefronts
    if h is not None:
        res = probe(L, h, 2, 1, nbytes, 8, 8, 0, 8, 24, 10, 1)
        if r > 0:
            probe_tb.append(res["tb_s"])
us = float(np.median(kernel_us))
print("plev kernel, %d members, 5 variables + mslp at %d levels: %d planes in, %d out, %.1f MB" % (M, len(LEVELS8), planes_in, planes_out,
                                                                                                   nbytes / 1e6))
print("  back to back on one stream: %.1f us per launch (max - min %.1f over %d rounds of %d)  %.2f TB/s" % (
    us, max(kernel_us) - min(kernel_us), rounds, launches, nbytes / us / 1e6), flush=True)
if probe_tb:
    tb = float(np.median(probe_tb))
    print("  streaming probe 2r:1w at the same bytes: %.2f TB/s (max - min %.2f)  -> the kernel reaches %.2f of it" % (
        tb, max(probe_tb) - min(probe_tb), nbytes / us / 1e6 / tb), flush=True)

if args.kernel_only:
    m.close()
    sys.exit(0)

# ---- (2) the cost of a sample ----
times = {v[0]: [] for v in VARIANTS}
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for name, variables, levels, every in VARIANTS:
        m.stats_configure([], 1)
        if levels:
            m.plev_configure(levels)
        m.stats_configure(variables or [], every or 1, False)
        m.run(36)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.calls):
            m.run(36)
        stop.record()
        stop.synchronize()
        if r > 0:
            times[name].append(start.elapsed_time(stop) / (36 * args.calls))
base = float(np.median(times["none"]))
print("%d members, %d calls of 36 steps per timing, %d rounds, mean only; groups: %d" % (M, args.calls, rounds, m.config()["chunks"]))
for name, _, _, _ in VARIANTS:
    t = float(np.median(times[name]))
    print("  %-34s %.4f ms per step (max - min %.4f)  %+6.2f %%" % (name, t, max(times[name]) - min(times[name]), 100.0 * (t / base - 1.0)),
          flush=True)
m.close()
