"""Cost of the in-loop quantile tape, 64 members, default plan: ms per model step in 360-step calls with an
event every 9 steps (six hours, 40 events per call) and every 36 steps (a day, 10 events per call), against the same model and
calls with the recorder off -- run from a checkout of the parent commit with its own library when --baseline-root names one, from
this tree otherwise.  Entries: the 10 / 50 / 90 % quantiles of z_plev at 500 hPa and the share of the members with convective
precipitation (two distinct planes, four planes of the ring).  Every timing is a process of its own, started by this one, which
never opens the GPU itself; the variants are alternated round by round in one session; medians over the rounds and the spread
(max - min) are reported, and the cost of an event above the baseline.  What to expect: the segment boundary alone costs
0.13 - 0.20 ms per event (profiles/breed_perf.txt); the front end transforms 64 members' planes; the point kernel is 18 workgroups
per distinct plane whose lanes order 64 values in the LDS (64 phases of 32 neighbour pairs).
Usage: perf_qtape.py [--members 64] [--rounds 7] [--calls 2] [--steps 360] [--baseline-root DIR] [--quick]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["off", "every 9", "every 36"]
ENTRIES = [("z_plev", 0, "quantile", 0.1), ("z_plev", 0, "quantile", 0.5), ("z_plev", 0, "quantile", 0.9), ("precnv", 0, "prob_above", 0.0)]


def worker(args):
    root = args.baseline_root if args.worker == "off" and args.baseline_root else ROOT
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
    m.plev_configure([500.0])
    m.run(36)
    note = "recorder off"
    if args.worker != "off":
        m.qtape_configure(ENTRIES, np.ones(args.members, dtype=np.int32), int(args.worker.split()[1]), capacity=64)
    m.run(args.steps)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.calls):
        m.run(args.steps)
    stop.record()
    stop.synchronize()
    if args.worker != "off":
        info = m.qtape_info()
        last = [m.qtape(k, info["held"] - 1, 1)[0].cpu().numpy() for k in range(len(ENTRIES))]
        note = "events %d members %d last: Z500 90 %% - 10 %% mean %.4g m, median mean %.6g m, wet share mean %.4g" % (
            info["applied"], info["members"], float((last[2] - last[0]).mean()), float(last[1].mean()), float(last[3].mean()))
    print("groups %d fold %d %s" % (m.config()["chunks"], m.config()["fold_geo"], note))
    print("ms_per_step %.6f" % (start.elapsed_time(stop) / (args.calls * args.steps)), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=64, help="members of the ensemble, all of them masked in")
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
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", v, "--members", str(args.members), "--calls", str(args.calls),
                   "--steps", str(args.steps)]
            if args.baseline_root:
                cmd += ["--baseline-root", os.path.abspath(args.baseline_root)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if done.returncode != 0:  # (a worker's own words, not a bare exit status)
                sys.exit("the worker '%s' failed with status %d:\n%s" % (v, done.returncode, done.stderr[-3000:]))
            out = done.stdout.splitlines()
            times[v].append(float([line for line in out if line.startswith("ms_per_step")][-1].split()[1]))
            notes[v] = [line for line in out if line.startswith("groups")][-1]
    lines = ["%d members, %d entries, %d calls of %d steps per timing, %d rounds, a process per timing; 'off' from %s" % (
        args.members, len(ENTRIES), args.calls, args.steps, rounds, "the parent commit's checkout" if args.baseline_root else "this tree")]
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
