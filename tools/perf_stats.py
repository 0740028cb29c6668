"""A/B of the time statistics' cost: ms per model step of 64 members in 36-step calls, without statistics and with all 8 variables
sampled every 1, 9 or 36 steps, mean only or with variance -- in the default plan (two member groups) and the serial one
(member_groups = 1).  All variants in one session, alternated round by round; the median over rounds is reported.
Usage: perf_stats.py [--members 64] [--rounds 7] [--calls 4] [--quick]   (--quick: one round, for a kernel trace)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyspeedy_amd  # noqa: E402
from pyspeedy_amd.model import EnsembleModel  # noqa: E402

VARS = ("u_grid", "v_grid", "t_grid", "q_grid", "phi_grid", "ps_grid", "precnv", "precls")
VARIANTS = (("none", None, False), ("every 1, variance", 1, True), ("every 9, variance", 9, True), ("every 9, mean only", 9, False),
            ("every 36, variance", 36, True), ("every 36, mean only", 36, False))

ap = argparse.ArgumentParser()
ap.add_argument("--members", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=4, help="36-step calls per timing")
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()
rounds = 1 if args.quick else args.rounds

sp = pyspeedy_amd.ModSpectral()
bc = np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))
plans = {}
for plan, groups in (("default", None), ("serial", 1)):
    m = EnsembleModel(sp, args.members)
    m.init_sst_anom(24)
    m.set_bc(bc)
    if groups:
        m.set_option("member_groups", groups)
    m.set_option("prepare_multi_step", 1)
    m.run(36)
    plans[plan] = m
torch.cuda.synchronize()
print("%d members, %s calls of 36 steps per timing, %d rounds; groups: default %d, serial %d" % (
    args.members, args.calls, rounds, plans["default"].config()["chunks"], 1), flush=True)

start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
times = {(p, v[0]): [] for p in plans for v in VARIANTS}
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for plan, m in plans.items():
        for name, every, variance in VARIANTS:
            m.stats_configure(VARS if every else [], every or 1, variance)
            m.run(36)
            torch.cuda.synchronize()
            start.record()
            for _ in range(args.calls):
                m.run(36)
            stop.record()
            stop.synchronize()
            if r > 0:
                times[(plan, name)].append(start.elapsed_time(stop) / (36 * args.calls))
for plan in plans:
    base = float(np.median(times[(plan, "none")]))
    print("plan %s" % plan)
    for name, every, variance in VARIANTS:
        t = float(np.median(times[(plan, name)]))
        spread = float(np.max(times[(plan, name)]) - np.min(times[(plan, name)]))
        print("  %-22s %.4f ms per step (max - min %.4f)  %+6.2f %%" % (name, t, spread, 100.0 * (t / base - 1.0)), flush=True)
# the reads, once per variable (for the kernel trace: the variance and ensemble kernels)
m = plans["default"]
m.stats_configure(VARS, 9, True)
m.run(36)
for n in VARS:
    m.stats_var(n)
    m.stats_ensemble(n)
torch.cuda.synchronize()
for m in plans.values():
    m.close()
