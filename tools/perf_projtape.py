"""Cost of the projection tape (weighted sums of single planes of the state's fields, formed behind the sampled steps and kept as
scalar series), 64 members, default plan: ms per model step in 360-step calls
    off                      no recorder
    tape (yardstick)         an fp32 tape of z_plev at 500 hPa and mslp, a sample every 9 steps: the same front end plus a store
    projection tape, small   the same two planes under 4 patterns each (8 entries), a sample every 9 steps
    projection tape, full    examples/climate_indices.py's entry list (7 entries on 5 planes under 5 patterns), a sample every 9 steps
The recorder's own cost is what lies above the yardstick.  Variants alternated round by round in one session; medians over the
rounds, every round's value and the spread (max - min) are reported.
Usage: perf_projtape.py [--members 64] [--rounds 7] [--calls 1] [--every 9] [--quick]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--members", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=1, help="360-step calls per timing")
ap.add_argument("--every", type=int, default=9)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()
rounds = 1 if args.quick else args.rounds
M, CALL = args.members, 360

spec = importlib.util.spec_from_file_location("climate_indices", os.path.join(ROOT, "examples", "climate_indices.py"))
example = importlib.util.module_from_spec(spec)
spec.loader.exec_module(example)

sp = pyspeedy_amd.ModSpectral()
pw = pyspeedy_amd.projection_weights(sp)
keys = list(example.PATTERNS)
full_weights = np.stack([getattr(pw, example.PATTERNS[k][0])(*example.PATTERNS[k][1]) for k in keys])
FULL = [(name, level, keys.index(pattern)) for _, _, _, parts in example.INDICES for name, level, pattern in parts]
small_weights = np.stack([pw.global_mean(), pw.box(150.0, -150.0, -40.0, 25.0), pw.point(11.3, 47.9),
                          np.random.default_rng(0).normal(0.0, 1.0, (48, 96))])
SMALL = [(name, 0, p) for name in ("z_plev", "mslp") for p in range(4)]

bc = np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))
m = EnsembleModel(sp, M)
m.init_sst_anom(24)
m.set_bc(bc)
m.set_option("prepare_multi_step", 1)
m.plev_configure([500.0])
m.run(36)
torch.cuda.synchronize()
steps = CALL * args.calls
start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed():
    torch.cuda.synchronize()
    start.record()
    for _ in range(args.calls):
        m.run(CALL)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


VARIANTS = ("off", "tape (yardstick)", "projection tape, small", "projection tape, full")
times = {v: [] for v in VARIANTS}
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for name in VARIANTS:
        m.tape_configure([], 1, 1)
        m.projtape_configure([], [], 1, 1)
        if name == "tape (yardstick)":
            m.tape_configure(["z_plev", "mslp"], args.every, 8)
        elif name == "projection tape, small":
            m.projtape_configure(small_weights, SMALL, args.every, 8)
        elif name == "projection tape, full":
            m.projtape_configure(full_weights, FULL, args.every, 8)
        m.run(36)
        t = timed()
        if r > 0:
            times[name].append(t)
m.tape_configure([], 1, 1)
m.projtape_configure([], [], 1, 1)
base, yard = float(np.median(times["off"])), float(np.median(times["tape (yardstick)"]))
print("%d members, groups: %d, a sample every %d steps, %d call(s) of %d steps per timing, %d rounds" % (
    M, m.config()["chunks"], args.every, args.calls, CALL, rounds))
for name in VARIANTS:
    t = float(np.median(times[name]))
    print("  %-24s %.4f ms per step (max - min %.4f)  %+6.2f %% over off  %+6.2f %% (%+.4f ms) over the yardstick  all rounds: %s" % (
        name, t, max(times[name]) - min(times[name]), 100.0 * (t / base - 1.0), 100.0 * (t / yard - 1.0), t - yard,
        " ".join("%.4f" % v for v in times[name])), flush=True)
m.close()
