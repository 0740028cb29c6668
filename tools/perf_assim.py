"""Cost of the in-loop assimilation, 64 members of which 63 assimilate, default plan: ms per model step in
360-step calls with an analysis every 9 steps (six hours, 40 events per call) and every 36 steps (a day, 10 events per call),
against the same calls with nothing configured -- run from a checkout of the parent commit with its own library when
--baseline-root names one, from this tree otherwise.  Every event has a row of observations: --entries lowest-level temperatures
under station stencils spread along 40 N, observed at the ensemble's initial mean with an error variance of 1 K^2.  Every timing is
a process of its own, started by this one, which never opens the GPU itself; the variants are alternated round by round in one
session; medians over the rounds and the spread (max - min) are reported, and the cost of an event above the baseline.  What to
expect: the segment boundary costs 0.13 - 0.20 ms per event (profiles/breed_perf.txt); the transform of 64 members reads
64 x 66 x 527 x 16 B = 36 MB and writes as much, tens of microseconds; the front end transforms 63 x 9 planes; the weights kernel
is one workgroup whose serial chain is --entries dependent rounds.
Usage: perf_assim.py [--members 64] [--entries 16] [--rounds 3] [--calls 2] [--steps 360] [--baseline-root DIR] [--quick]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["baseline", "every 9", "every 36"]


def worker(args):
    root = args.baseline_root if args.worker == "baseline" and args.baseline_root else ROOT
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel
    sp = pyspeedy_amd.ModSpectral()
    bc = np.load(os.path.join(root, "pyspeedy_amd", "data", "example_bc.npz"))
    m = EnsembleModel(sp, args.members)
    m.init_sst_anom(24)
    m.set_bc(bc)
    m.set_option("prepare_multi_step", 1)
    for i in range(1, args.members):  # a different temperature per member, as the tests perturb
        f = 1.0 + 2e-4 * np.random.default_rng(i).standard_normal((31, 32, 8, 1))
        f[0] = 1.0
        m.set("t", m.get("t", i) * f, i)
    m.run(36)
    note = "nothing configured"
    if args.worker != "baseline":
        every = int(args.worker.split()[1])
        pw = pyspeedy_amd.projection_weights(sp)
        maps = np.stack([pw.point(360.0 * k / args.entries + 1.0, 40.0) for k in range(args.entries)])
        entries = [("t_grid", 7, k) for k in range(args.entries)]
        mask = np.ones(args.members, dtype=np.int32)
        mask[0] = 0
        m.assim_configure(maps, entries, mask, every, capacity=64)
        yo = m.assim_compute().cpu().numpy().mean(axis=1)
        last = m.current_step + (1 + args.calls) * args.steps
        stamps = [n for n in range(m.current_step + 1, last + 1) if n % every == 0]
        m.assim_observations(stamps, np.tile(yo, (len(stamps), 1)), 1.0)
    m.run(args.steps)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.calls):
        m.run(args.steps)
    stop.record()
    stop.synchronize()
    if args.worker != "baseline":
        info = m.assim_info()
        used = int(m.assim()["used"].sum().item())
        note = "events %d skipped %d entries used in the held events %d" % (info["applied"], info["skipped"], used)
    print("groups %d fold %d %s" % (m.config()["chunks"], m.config()["fold_geo"], note))
    print("ms_per_step %.6f" % (start.elapsed_time(stop) / (args.calls * args.steps)), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--entries", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2, help="calls per timing")
    ap.add_argument("--steps", type=int, default=360, help="steps per call")
    ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit for the baseline (default: this tree)")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    import numpy as np
    rounds = 1 if args.quick else args.rounds
    times, notes = {v: [] for v in VARIANTS}, {}
    for r in range(rounds):
        for v in VARIANTS:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", v, "--members", str(args.members), "--entries", str(args.entries),
                   "--calls", str(args.calls), "--steps", str(args.steps)]
            if args.baseline_root:
                cmd += ["--baseline-root", os.path.abspath(args.baseline_root)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if done.returncode != 0:  # (a worker's own words, not a bare exit status)
                sys.exit("the worker '%s' failed with status %d:\n%s" % (v, done.returncode, done.stderr[-3000:]))
            out = done.stdout.splitlines()
            times[v].append(float([line for line in out if line.startswith("ms_per_step")][-1].split()[1]))
            notes[v] = [line for line in out if line.startswith("groups")][-1]
    print("%d members (%d assimilate), %d entries, %d calls of %d steps per timing, %d rounds, a process per timing; baseline from %s" % (
        args.members, args.members - 1, args.entries, args.calls, args.steps, rounds, "the parent commit's checkout" if args.baseline_root else "this tree"))
    base = float(np.median(times["baseline"]))
    for v in VARIANTS:
        t = float(np.median(times[v]))
        line = "  %-9s %.4f ms per step (max - min %.4f)" % (v, t, max(times[v]) - min(times[v]))
        if v != "baseline":
            line += "  %+.1f us per event over the baseline" % (1e3 * (t - base) * int(v.split()[1]))
        print(line + "  all rounds: %s  (%s)" % (" ".join("%.4f" % x for x in times[v]), notes[v]), flush=True)


if __name__ == "__main__":
    main()
