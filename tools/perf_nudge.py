"""Cost of in-loop nudging (relaxation of the spectral state toward targets behind every step), 64 members, default plan: ms per
model step in 360-step calls
    parent, off     the parent commit's library (--parent-lib, a build of the commit before nudging existed), nothing configured
    off             this build, nothing configured: the launches of the parent
    vor div t       this build, vor, div and t nudged at l <= 15, tau = 6 h, six-hourly targets
    all five        this build, all five names nudged at every l <= 31 (the largest launch there is), six-hourly targets
A library is chosen when the package is imported (PYSPEEDY_AMD_LIB), so every timing is a process of its own, started by this
one, which never opens the GPU itself; the variants are alternated round by round in one session; medians over the rounds and the
spread (max - min) are reported.  The expectation to compare with is the byte ratio only: the full set reads and writes 1.1 MB per
member and step against the step's 20 MB, +5.5 % algorithmic bytes.
Usage: perf_nudge.py [--members 64] [--rounds 5] [--calls 2] [--steps 360] [--parent-lib PATH] [--quick]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("parent, off", "off", "vor div t", "all five")


def worker(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import pyspeedy_amd
    import pyspeedy_amd._lib as L
    from pyspeedy_amd.model import EnsembleModel
    if args.worker == "parent, off":  # (the parent's library does not have the nudging symbols: do not ask it for them)
        for name in [n for n in L._SIGNATURES if n.startswith("spd_model_nudge_")]:
            del L._SIGNATURES[name]
    sp = pyspeedy_amd.ModSpectral()
    bc = np.load(os.path.join(ROOT, "pyspeedy_amd", "data", "example_bc.npz"))
    m = EnsembleModel(sp, args.members)
    m.init_sst_anom(24)
    m.set_bc(bc)
    m.set_option("prepare_multi_step", 1)
    if args.worker in ("vor div t", "all five"):
        names = ("vor", "div", "t") if args.worker == "vor div t" else EnsembleModel.NUDGE_NAMES
        l_max = 15 if args.worker == "vor div t" else 31
        stamps = list(range(0, 36 + (args.calls + 1) * args.steps + 9, 9))  # six-hourly targets over the whole run
        gains = {n: pyspeedy_amd.nudge_gains(6.0, levels=1 if n == "ps" else None, l_max=l_max) for n in names}
        m.nudge_configure(gains, capacity=len(stamps))
        state = {n: m.get(n)[..., 0] for n in names}  # (the target: the state at rest, in every slot)
        m.nudge_targets(stamps, {n: np.broadcast_to(state[n], (len(stamps),) + state[n].shape) for n in names})
    m.run(36)
    m.run(args.steps)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.calls):
        m.run(args.steps)
    stop.record()
    stop.synchronize()
    print("groups %d fold %d" % (m.config()["chunks"], m.config()["fold_geo"]))
    print("ms_per_step %.6f" % (start.elapsed_time(stop) / (args.calls * args.steps)), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
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
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout.splitlines()
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
