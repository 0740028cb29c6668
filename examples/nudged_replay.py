#!/usr/bin/env python3
"""Replay a truth run: half of a perturbed ensemble is nudged toward it inside one multi-day device call.

A single "truth" member runs first; its vorticity, divergence and temperature every six hours become the targets.  Then an
ensemble whose members start from a perturbed temperature runs the same days as ONE call.  Half of the members are relaxed toward
the truth's large scales (total wavenumber l <= --l-max, time scale --tau hours) after every step, on the device, between the
six-hourly targets by linear interpolation; the other half is left free through the member mask.  The script prints, per day, the
rms distance of the 500 hPa height to the truth for the two halves.

    python examples/nudged_replay.py [--members 16] [--days 5] [--tau 6] [--l-max 15] [--noise 0.01]

API surface used: pyspeedy_amd.nudge_gains, EnsembleModel.nudge_configure / nudge_targets / nudge_info, tape_configure / tape (the
six-hourly Z500 of every member, recorded inside the call), plev_configure, run_checked, device_view + grid2spectral for the
perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ("vor", "div", "t")
TARGET_EVERY = 9  # model steps of 40 minutes: six hours
LEVELS_HPA = (500.0,)


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])

    def at_least(n):
        def conv(text):
            v = int(text)
            if v < n:
                raise argparse.ArgumentTypeError("must be at least %d" % n)
            return v
        return conv

    def tau(text):
        v = float(text)
        if v < 2.0 / 3.0:
            raise argparse.ArgumentTypeError("must be at least one step of 40 minutes (2/3 h)")
        return v

    p.add_argument("--members", type=at_least(2), default=16, help="ensemble size (a nudged and a free half)")
    p.add_argument("--days", type=at_least(1), default=5, help="days to simulate, as one device call")
    p.add_argument("--tau", type=tau, default=6.0, help="relaxation time scale [h]")
    p.add_argument("--l-max", type=at_least(0), default=15, help="largest total wavenumber that is nudged")
    p.add_argument("--noise", type=float, default=0.01, help="standard deviation of the temperature perturbation [K]")
    return p.parse_args(argv)


def main():
    args = parse()
    import torch
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel

    sp = pyspeedy_amd.ModSpectral(0)
    bc = np.load(os.path.join(os.path.dirname(pyspeedy_amd.__file__), "data", "example_bc.npz"))
    steps = 36 * args.days
    stamps = list(range(0, steps + 1, TARGET_EVERY))

    # the truth: one member, its spectral state every six hours (time level 1, the level the exports show) and its Z500
    truth = EnsembleModel(sp, 1)
    truth.set_bc(bc)
    truth.plev_configure(LEVELS_HPA)
    truth.tape_configure(["z_plev"], TARGET_EVERY, len(stamps), dtype="float64")
    fields = {n: [truth.get(n)[..., 0]] for n in NAMES}
    for _ in stamps[1:]:
        truth.run(TARGET_EVERY)
        for n in NAMES:
            fields[n].append(truth.get(n)[..., 0])
    z_truth = truth.tape("z_plev")[0, :, 0]  # [samples, lat, lon]
    truth.close()

    # the ensemble: perturbed temperatures; the first half is nudged, the second is free
    model = EnsembleModel(sp, args.members)
    model.set_bc(bc)
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng(i).normal(0.0, args.noise, (96, 48, 8)).transpose(2, 1, 0)
                      for i in range(args.members)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()
    nudged = np.arange(args.members) < args.members // 2
    gains = pyspeedy_amd.nudge_gains(args.tau, l_max=args.l_max)
    model.nudge_configure({n: gains for n in NAMES}, members=nudged, capacity=len(stamps))
    model.nudge_targets(stamps, {n: np.stack(fields[n]) for n in NAMES})
    model.plev_configure(LEVELS_HPA)
    model.tape_configure(["z_plev"], TARGET_EVERY, len(stamps), dtype="float64")
    failed, _ = model.run_checked(steps)  # one device call: every step is nudged and checked on the device
    if (failed >= 0).any():
        raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())

    info = model.nudge_info()
    z = model.tape("z_plev")[:, :, 0]  # [M, samples, lat, lon]
    lat = torch.from_numpy(np.asarray(sp.table("radang"), dtype=np.float64)).to(z.device)
    w = torch.cos(lat)
    diff2 = ((z - z_truth[None]) ** 2).mean(dim=3)                      # zonal mean of the squared distance
    rms = torch.sqrt((diff2 * w).sum(dim=2) / w.sum()).cpu().numpy()    # [M, samples]: area-weighted rms
    times = model.tape_times()
    print("%d members, %d of them nudged (l <= %d, tau = %g h), %d steps nudged, %d targets" % (
        args.members, int(nudged.sum()), args.l_max, args.tau, info["applied"], info["in_use"]))
    print("  date               rms Z500 distance to the truth [m]:  nudged half    free half")
    for k, when in enumerate(times):
        if (k + 1) % 4 == 0:  # (daily)
            print("  %s   %44.4f   %10.4f" % (when.strftime("%Y-%m-%d %H:%M"), rms[nudged, k].mean(), rms[~nudged, k].mean()))
    model.close()


if __name__ == "__main__":
    main()
