"""Cost of in-loop breeding (member perturbations rescaled against a control run at the segment ends of a multi-step call), 64
members -- member 0 the control, 63 bred -- default plan: ms per model step in 360-step calls
    parent, off     the parent commit's library (--parent-lib, a build of the commit before breeding existed), nothing configured
    off             this build, nothing configured: the launches of the parent
    every 9         this build, a rescale every 9 steps (six hours): 40 segments per call
    every 36        this build, a rescale every 36 steps (a day): 10 segments per call
A library is chosen when the package is imported (PYSPEEDY_AMD_LIB), so every timing is a process of its own, started by this
one, which never opens the GPU itself; the variants are alternated round by round in one session; medians over the rounds and the
spread (max - min) are reported.  The expectation to compare with is the byte ratio: roughly 3 MB per bred member and event (two
members' time level 1 read for the norm, both time levels of both read and the bred member's written for the rescale) against
20 MB per member and step, under 1 % at every = 9; what a segment end adds on top is the join and fork of the group streams.
Usage: perf_breed.py [--members 64] [--rounds 3] [--calls 2] [--steps 360] [--parent-lib PATH] [--quick]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("parent, off", "off", "every 9", "every 36")


def worker(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import pyspeedy_amd
    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    if args.worker == "parent, off":  # (the parent's library does not have the breeding symbols: do not ask it for them)
        for name in [n for n in L._SIGNATURES if n.startswith("spd_model_breed_") or n == "spd_breed_check"]:
            del L._SIGNATURES[name]
    sp = pyspeedy_amd.ModSpectral()
    bc = np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))
    m = EnsembleModel(sp, args.members)
    m.init_sst_anom(24)
    m.set_bc(bc)
    m.set_option("prepare_multi_step", 1)
    if args.worker.startswith("every"):
        for i in range(1, args.members):  # a different temperature per bred member, as the tests perturb
            f = 1.0 + 2e-4 * np.random.default_rng(i).standard_normal((31, 32, 8, 1))
            f[0] = 1.0
            m.set("t", m.get("t", i) * f, i)
    m.run(36)
    if args.worker.startswith("every"):  # the target: the kinetic-energy amplitude the perturbations have after the first day
        control = np.zeros(args.members, dtype=np.int32)
        control[0] = -1
        m.breed_configure(control, 1.0, int(args.worker.split()[1]), capacity=64, in_loop=False)
        target = float(m.breed_amplitude()[1:].mean())
        m.breed_configure(control, target, int(args.worker.split()[1]), capacity=64)
    m.run(args.steps)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.calls):
        m.run(args.steps)
    stop.record()
    stop.synchronize()
    applied = m.breed_info()["applied"] if args.worker != "parent, off" else 0
    print("groups %d fold %d rescales %d" % (m.config()["chunks"], m.config()["fold_geo"], applied))
    print("ms_per_step %.6f" % (start.elapsed_time(stop) / (args.calls * args.steps)), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2, help="calls per timing")
    ap.add_argument("--steps", type=int, default=360, help="steps per call")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "build_variants", "libpyspeedy_amd_parent.so"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    import numpy as np
    variants = [v for v in VARIANTS if v != "parent, off" or os.path.isfile(args.parent_lib)]
    if "parent, off" not in variants:
        print("(no parent library at %s: the parent line is left out)" % args.parent_lib)
    rounds = 1 if args.quick else args.rounds
    times, groups = {v: [] for v in variants}, ""
    for r in range(rounds):
        for name in variants:
            env = dict(os.environ)
            env.pop("PYSPEEDY_AMD_LIB", None)
            if name == "parent, off":
                env["PYSPEEDY_AMD_LIB"] = args.parent_lib
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", name, "--members", str(args.members), "--calls", str(args.calls),
                   "--steps", str(args.steps)]
            done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if done.returncode != 0:  # (a worker's own words, not a bare exit status)
                sys.exit("the worker '%s' failed with status %d:\n%s" % (name, done.returncode, done.stderr[-3000:]))
            out = done.stdout.splitlines()
            times[name].append(float([line for line in out if line.startswith("ms_per_step")][-1].split()[1]))
            groups = [line for line in out if line.startswith("groups")][-1]
    base = float(np.median(times["off"]))
    print("%d members (%s of the last worker), %d calls of %d steps per timing, %d rounds, a process per timing" % (
        args.members, groups, args.calls, args.steps, rounds))
    for name in variants:
        t = float(np.median(times[name]))
        print("  %-12s %.4f ms per step (max - min %.4f)  %+6.2f %% over off  all rounds: %s" % (
            name, t, max(times[name]) - min(times[name]), 100.0 * (t / base - 1.0), " ".join("%.4f" % v for v in times[name])), flush=True)


if __name__ == "__main__":
    main()
