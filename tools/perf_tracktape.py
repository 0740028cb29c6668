"""Cost of the track tape (the extreme of single planes of the state's fields over regions and where it lies, followed from sample
to sample, formed behind the sampled steps), 64 members, default plan: ms per model step in 360-step calls
    off                      no recorder
    tape (yardstick)         an fp32 tape of the same planes -- mslp, z_plev at 500 hPa, precnv: the same front end plus a store
    projection tape          the same planes under the same regions as weight maps (3 entries): the same front end plus a sum
    track tape               the mslp minimum of a North-Atlantic box (radius 2), the z_plev minimum of the same box at 500 hPa
                             (radius 2) and the precnv maximum of the tropical band (radius 0)
each of the three recorders with a sample every 9 and every 36 steps.  The recorder's own cost is what lies above the yardstick.
Variants alternated round by round in one session; medians over the rounds, every round's value and the spread (max - min) are
reported.
Usage: perf_tracktape.py [--members 64] [--rounds 7] [--calls 1] [--quick]"""
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
ap.add_argument("--calls", type=int, default=1, help="360-step calls per timing")
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()
rounds = 1 if args.quick else args.rounds
M, CALL = args.members, 360
EVERY = (9, 36)

sp = pyspeedy_amd.ModSpectral()
pw = pyspeedy_amd.projection_weights(sp)
regions = np.stack([pw.box(280.0, 350.0, 30.0, 70.0), pw.band(-20.0, 20.0)])
PLANES = ["precnv", "z_plev", "mslp"]
TRACK = [("mslp", 0, 0, "min", 2), ("z_plev", 0, 0, "min", 2), ("precnv", 0, 1, "max", 0)]
PROJ = [(name, level, region) for name, level, region, _, _ in TRACK]

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


def all_off():
    m.tape_configure([], 1, 1)
    m.projtape_configure([], [], 1, 1)
    m.tracktape_off()


VARIANTS = [("off", None, 0)] + [(kind, kind, every) for every in EVERY for kind in ("tape (yardstick)", "projection tape", "track tape")]
label = {v: v[0] if v[1] is None else "%s, every %d" % (v[0], v[2]) for v in VARIANTS}
times = {v: [] for v in VARIANTS}
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for v in VARIANTS:
        _, kind, every = v
        all_off()
        if kind == "tape (yardstick)":
            m.tape_configure(PLANES, every, 8)
        elif kind == "projection tape":
            m.projtape_configure(regions, PROJ, every, 8)
        elif kind == "track tape":
            m.tracktape_configure(regions, TRACK, every, 8)
        m.run(36)
        t = timed()
        if r > 0:
            times[v].append(t)
all_off()
base = float(np.median(times[VARIANTS[0]]))
print("%d members, groups: %d, %d call(s) of %d steps per timing, %d rounds" % (M, m.config()["chunks"], args.calls, CALL, rounds))
for v in VARIANTS:
    t = float(np.median(times[v]))
    yard = base if v[1] is None else float(np.median(times[("tape (yardstick)", "tape (yardstick)", v[2])]))
    per_sample = 0.0 if v[1] is None else (t - base) * v[2]
    print("  %-28s %.4f ms per step (max - min %.4f)  %+6.2f %% over off  %+.4f ms over the yardstick  %.4f ms per sampled step over "
          "off  all rounds: %s" % (label[v], t, max(times[v]) - min(times[v]), 100.0 * (t / base - 1.0), t - yard, per_sample,
                                    " ".join("%.4f" % x for x in times[v])), flush=True)
m.close()
