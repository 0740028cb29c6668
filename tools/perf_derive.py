"""Cost of the derived fields on the device, 64 members: (1) spd_model_derive_compute of all fourteen names at 8 levels from the grid
arrays (the 18 transforms of vor, div and grad ln ps per member, then the two launches of derive_kernel) and of vor_grid / div_grid
alone (the transforms only), back to back on one stream, timed by events; the difference is the kernel pair, given in microseconds
and TB/s over its algorithmic bytes next to what the streaming probe moves in the 2 reads : 1 write shape at the same size in the
same session; (2) ms per model step in 36-step calls with nothing configured, with omega_plev at 500 hPa alone on an fp32 tape, and
with the set of examples/moisture_transport.py (omega_plev at 500 hPa and tcwv on an fp32 tape, a tcwv box mean on the projection
tape, monthly means of ivt_u / ivt_v on the window tape), sampled every 9 or 36 steps.  Variants alternated round by round in one
session; medians over the rounds and the spread (max - min) are reported.
Usage: perf_derive.py [--members 64] [--rounds 7] [--calls 4] [--quick] [--kernel-only]   (--quick: one round; --kernel-only: part
(1) alone, for `rocprofv3 --kernel-trace --stats`)"""
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
BOX = np.zeros((1, 48, 96))
BOX[0, 20:30, 10:40] = 1.0 / 300.0
VARIANTS = [("none", None, None)]
for every in (9, 36):
    VARIANTS += [("omega_plev at 500 hPa, every %d" % every, "omega", every), ("the example's set, every %d" % every, "example", every)]

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

# ---- (1) the stand-alone call ----
m.plev_configure(LEVELS8)
m.derived()  # (allocates the results, refreshes the grid arrays)
L, stream = m._lib, m._stream()
none = (C.c_char_p * 1)()
two = (C.c_char_p * 2)(b"vor_grid", b"div_grid")
n = len(LEVELS8)
planes_in = 6 * 8 + 3                      # u, v, T, q, vor, div | ps, px, py, each counted once
planes_read = (3 * 8 + 3) + (6 * 8 + 1)    # as the two launches read them
planes_out = 3 * 8 + 4 + 5 * n
nbytes = (planes_in + planes_out) * M * 4608 * 8
launches = 20
all_us, xf_us, probe_tb = [], [], []
h = sp._h


def timed(names, count):
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        _lib.check(L.spd_model_derive_compute(m._m, names, count, 0, M, 0, stream), "spd_model_derive_compute")
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / launches


for r in range(rounds + 1):
    a, x = timed(none, 0), timed(two, 2)
    if r > 0:
        all_us.append(a)
        xf_us.append(x)
    if h is not None:
        res = probe(L, h, 2, 1, nbytes, 8, 8, 0, 8, 24, 10, 1)
        if r > 0:
            probe_tb.append(res["tb_s"])
a, x = float(np.median(all_us)), float(np.median(xf_us))
us = a - x
print("derived fields, %d members, fourteen names at %d levels: %d planes in (%d as the two launches read them), %d out, %.1f MB "
      "algorithmic" % (M, n, planes_in, planes_read, planes_out, nbytes / 1e6))
print("  all names, back to back on one stream: %.1f us per call (max - min %.1f over %d rounds of %d)" % (
    a, max(all_us) - min(all_us), rounds, launches))
print("  vor_grid, div_grid alone (the %d transforms): %.1f us per call (max - min %.1f)" % (18 * M, x, max(xf_us) - min(xf_us)))
print("  -> the two launches of derive_kernel: %.1f us  %.2f TB/s over the algorithmic bytes" % (us, nbytes / us / 1e6), flush=True)
if probe_tb:
    tb = float(np.median(probe_tb))
    print("  streaming probe 2r:1w at the same bytes: %.2f TB/s (max - min %.2f)  -> the kernel pair reaches %.2f of it" % (
        tb, max(probe_tb) - min(probe_tb), nbytes / us / 1e6 / tb), flush=True)

if args.kernel_only:
    m.close()
    sys.exit(0)


# ---- (2) the cost of a sample ----
def configure(kind, every):
    m.tape_configure([], 1, 1)
    m.projtape_configure(BOX, [], 1, 1)
    m.wintape_configure([], 36, 1)
    if kind is None:
        return
    m.plev_configure([500.0])
    m.tape_configure(["omega_plev"] if kind == "omega" else ["omega_plev", "tcwv"], every, 4, dtype="float32")
    if kind == "example":
        m.projtape_configure(BOX, [("tcwv", 0, 0)], every, 4)
        m.wintape_configure([("ivt_u", "mean"), ("ivt_v", "mean")], "month", 2, sample_every=every)


times = {v[0]: [] for v in VARIANTS}
for r in range(rounds + 1):  # (round 0: warm-up, not counted)
    for name, kind, every in VARIANTS:
        configure(kind, every)
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
print("%d members, %d calls of 36 steps per timing, %d rounds; groups: %d" % (M, args.calls, rounds, m.config()["chunks"]))
for name, _, _ in VARIANTS:
    t = float(np.median(times[name]))
    print("  %-34s %.4f ms per step (max - min %.4f)  %+6.2f %%" % (name, t, max(times[name]) - min(times[name]), 100.0 * (t / base - 1.0)),
          flush=True)
m.close()
