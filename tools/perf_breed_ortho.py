"""Cost of orthonormalised breeding against plain breeding (section 4i) at the same rescale steps, 64 members,
default plan: ms per model step in 360-step calls, member 0 the control of
    63 bred    members 1 ... 63: one family of 63
    15 bred    members 1 ... 15: one family of 15; the other 48 members run free
each with a rescale every 9 steps (six hours, 40 events per call) and every 36 steps (a day, 10 events per call), plain and
orthonormalised.  Every timing is a process of its own, started by this one, which never opens the GPU itself; the variants are
alternated round by round in one session; medians over the rounds and the spread (max - min) are reported, and the cost of an
event above plain breeding's.  What to expect: the segment boundary costs 0.13 - 0.20 ms per event with plain breeding
(profiles/breed_perf.txt); the Gram, factor and transform launches of a family of 63 move about 70 MB and 0.6 GFLOP, tens of
microseconds, of which the factor's dependent chain (one workgroup) is the longest part.
Usage: perf_breed_ortho.py [--members 64] [--rounds 3] [--calls 2] [--steps 360] [--quick]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(bred, every, kind) for bred in (63, 15) for every in (9, 36) for kind in ("plain", "ortho")]


def worker(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel
    bred, every, kind = args.worker.split(",")
    bred, every = min(int(bred), args.members - 1), int(every)
    sp = pyspeedy_amd.ModSpectral()
    bc = np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))
    m = EnsembleModel(sp, args.members)
    m.init_sst_anom(24)
    m.set_bc(bc)
    m.set_option("prepare_multi_step", 1)
    for i in range(1, args.members):  # a different temperature per member, as the tests perturb
        f = 1.0 + 2e-4 * np.random.default_rng(i).standard_normal((31, 32, 8, 1))
        f[0] = 1.0
        m.set("t", m.get("t", i) * f, i)
    m.run(36)
    control = np.full(args.members, -1, dtype=np.int32)
    control[1:bred + 1] = 0
    m.breed_configure(control, 1.0, every, capacity=64, in_loop=False)
    target = float(m.breed_amplitude()[1:bred + 1].mean())
    m.breed_configure(control, target, every, capacity=64, orthogonalize=kind == "ortho")
    m.run(args.steps)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.calls):
        m.run(args.steps)
    stop.record()
    stop.synchronize()
    info = m.breed_info()
    left_alone = int((m.breed()["amplitude"].cpu().numpy()[:, 1:bred + 1] == 0.0).sum())
    print("groups %d fold %d rescales %d left alone %d" % (m.config()["chunks"], m.config()["fold_geo"], info["applied"], left_alone))
    print("ms_per_step %.6f" % (start.elapsed_time(stop) / (args.calls * args.steps)), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2, help="calls per timing")
    ap.add_argument("--steps", type=int, default=360, help="steps per call")
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
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "%d,%d,%s" % v, "--members", str(args.members), "--calls", str(args.calls),
                   "--steps", str(args.steps)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if done.returncode != 0:  # (a worker's own words, not a bare exit status)
                sys.exit("the worker '%s' failed with status %d:\n%s" % (v, done.returncode, done.stderr[-3000:]))
            out = done.stdout.splitlines()
            times[v].append(float([line for line in out if line.startswith("ms_per_step")][-1].split()[1]))
            notes[v] = [line for line in out if line.startswith("groups")][-1]
    print("%d members, %d calls of %d steps per timing, %d rounds, a process per timing" % (args.members, args.calls, args.steps, rounds))
    for bred, every, kind in VARIANTS:
        t = float(np.median(times[bred, every, kind]))
        line = "  %2d bred, every %2d, %-5s %.4f ms per step (max - min %.4f)" % (bred, every, kind, t, max(times[bred, every, kind]) - min(times[bred, every, kind]))
        if kind == "ortho":
            line += "  %+.1f us per event over plain" % (1e3 * (t - float(np.median(times[bred, every, "plain"]))) * every)
        print(line + "  all rounds: %s  (%s)" % (" ".join("%.4f" % x for x in times[bred, every, kind]), notes[bred, every, kind]), flush=True)


if __name__ == "__main__":
    main()
