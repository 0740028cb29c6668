"""Cost of the in-loop verification tape, 65 members of which 64 are scored against the 65th, default plan:
ms per model step in 360-step calls with an event every 9 steps (six hours, 40 events per call) and every 36 steps (a day, 10
events per call), against the same model and calls with the recorder off -- run from a checkout of the parent commit with its own
library when --baseline-root names one, from this tree otherwise.  --entries entries: t_plev at 850 hPa and z_plev at 500 hPa under
three zonal bands each (the scores of examples/osse_scores.py), further ones t_grid levels under the global mean.  Every timing is a
process of its own, started by this one, which never opens the GPU itself; the variants are alternated round by round in one
session; medians over the rounds and the spread (max - min) are reported, and the cost of an event above the baseline.  What to
expect: the segment boundary alone costs 0.13 - 0.20 ms per event (profiles/breed_perf.txt); the front end transforms 65 members'
planes; the point kernel is 18 workgroups per distinct plane whose lanes run a dependent chain of r (r - 1) / 2 = 2016 additions;
the reduce kernel is one workgroup per entry.
Usage: perf_verif.py [--members 64] [--entries 6] [--rounds 7] [--calls 2] [--steps 360] [--baseline-root DIR] [--quick]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["off", "every 9", "every 36"]


def worker(args):
    root = args.baseline_root if args.worker == "off" and args.baseline_root else ROOT
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel
    sp = pyspeedy_amd.ModSpectral()
    bc = np.load(os.path.join(root, "pyspeedy_amd", "data", "example_bc.npz"))
    members = args.members + 1  # the truth is one more member
    m = EnsembleModel(sp, members)
    m.init_sst_anom(24)
    m.set_bc(bc)
    m.set_option("prepare_multi_step", 1)
    for i in range(1, members):  # a different temperature per member, as the tests perturb
        f = 1.0 + 2e-4 * np.random.default_rng(i).standard_normal((31, 32, 8, 1))
        f[0] = 1.0
        m.set("t", m.get("t", i) * f, i)
    m.plev_configure([850.0, 500.0])
    m.run(36)
    note = "recorder off"
    if args.worker != "off":
        every = int(args.worker.split()[1])
        pw = pyspeedy_amd.projection_weights(sp)
        maps = np.stack([pw.band(20.0, 90.0), pw.band(-20.0, 20.0), pw.band(-90.0, -20.0), pw.global_mean()])
        entries = ([("t_plev", 0, g) for g in range(3)] + [("z_plev", 1, g) for g in range(3)] + [("t_grid", k % 8, 3) for k in range(250)])
        mask = np.ones(members, dtype=np.int32)
        mask[-1] = 0
        m.verif_configure(maps, entries[:args.entries], mask, members - 1, every, capacity=64)
    m.run(args.steps)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.calls):
        m.run(args.steps)
    stop.record()
    stop.synchronize()
    if args.worker != "off":
        info = m.verif_info()
        crps = m.verif()["crps"][-1, 0].cpu().numpy()
        note = "events %d scored members %d last crps %s" % (info["applied"], info["members"], " ".join("%.4g" % x for x in crps[:6]))
    print("groups %d fold %d %s" % (m.config()["chunks"], m.config()["fold_geo"], note))
    print("ms_per_step %.6f" % (start.elapsed_time(stop) / (args.calls * args.steps)), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=64, help="members that are scored (one more is the truth)")
    ap.add_argument("--entries", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2, help="calls per timing")
    ap.add_argument("--steps", type=int, default=360, help="steps per call")
    ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit for the variant 'off' (default: this tree)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
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
    lines = ["%d members scored against one more, %d entries, %d calls of %d steps per timing, %d rounds, a process per timing; 'off' from %s" % (
        args.members, args.entries, args.calls, args.steps, rounds, "the parent commit's checkout" if args.baseline_root else "this tree")]
    base = float(np.median(times["off"]))
    for v in VARIANTS:
        t = float(np.median(times[v]))
        line = "  %-9s %.4f ms per step (max - min %.4f)" % (v, t, max(times[v]) - min(times[v]))
        if v != "off":
            line += "  %+.1f us per event over off" % (1e3 * (t - base) * int(v.split()[1]))
        lines.append(line + "  all rounds: %s  (%s)" % (" ".join("%.4f" % x for x in times[v]), notes[v]))
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
