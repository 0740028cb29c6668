#!/usr/bin/env python3
"""Breed perturbations against a control run inside one multi-day device call and print their growth rates.

Member 0 is the control; every other member starts from it with a small random temperature perturbation and runs a first day
freely; the mean amplitude the perturbations have then is the target.  From there on, every --every steps
(9 steps of 40 minutes: six hours) the perturbation of each member is pulled back to that amplitude in the chosen norm, on
the device, between the steps of ONE run_checked() call: X_p <- X_c + s (X_p - X_c), s = target / A.  The amplitude A a
perturbation had grown to before each rescale is kept in a ring; ln(A / target) over the cycle length is the growth rate of the
bred vector, which settles within a few days on the rate of the fastest-growing large-scale instabilities.

    python examples/bred_vectors.py [--members 8] [--days 10] [--every 9] [--norm kinetic_energy] [--noise 0.01]

API surface used: pyspeedy_amd.breed_weights, EnsembleModel.breed_configure / breed_amplitude / breed / breed_times / breed_growth /
breed_info, run_checked, device_view + grid2spectral for the perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NORMS = ("kinetic_energy", "total_energy", "t_rms")


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])

    def at_least(n):
        def conv(text):
            v = int(text)
            if v < n:
                raise argparse.ArgumentTypeError("must be at least %d" % n)
            return v
        return conv

    p.add_argument("--members", type=at_least(2), default=8, help="ensemble size: one control and members - 1 bred members")
    p.add_argument("--days", type=at_least(1), default=10, help="days to simulate, as one device call")
    p.add_argument("--every", type=at_least(1), default=9, help="model steps of 40 minutes between two rescales (9: six hours)")
    p.add_argument("--norm", choices=NORMS, default="kinetic_energy", help="the norm the amplitude is measured in")
    p.add_argument("--noise", type=float, default=0.01, help="standard deviation of the initial temperature perturbation [K]")
    return p.parse_args(argv)


def control_of(members):
    """member 0 is the control of all others"""
    control = np.zeros(members, dtype=np.int32)
    control[0] = -1
    return control


def main():
    args = parse()
    import torch
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel

    sp = pyspeedy_amd.ModSpectral(0)
    bc = np.load(os.path.join(os.path.dirname(pyspeedy_amd.__file__), "data", "example_bc.npz"))
    model = EnsembleModel(sp, args.members)
    model.set_bc(bc)
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.zeros((8, 48, 96)) if i == 0 else
                      np.random.default_rng(i).normal(0.0, args.noise, (96, 48, 8)).transpose(2, 1, 0) for i in range(args.members)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()

    steps = 36 * args.days
    events = steps // args.every
    weights = pyspeedy_amd.breed_weights(args.norm)
    # the target: the mean amplitude of the perturbations after a first day without rescaling (a temperature perturbation of a
    # state at rest has no kinetic energy yet), measured before anything is rescaled
    model.run(36)
    model.breed_configure(control_of(args.members), 1.0, args.every, weights=weights, capacity=max(events, 1), in_loop=False)
    target = float(model.breed_amplitude()[1:].mean())
    model.breed_configure(control_of(args.members), target, args.every, weights=weights, capacity=max(events, 1))
    failed, _ = model.run_checked(steps)  # one device call: every step checked, every cycle rescaled on the device
    if (failed >= 0).any():
        raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())

    info = model.breed_info()
    growth = model.breed_growth()[:, 1:] * 86400.0  # [events][bred members], per day
    amplitude = model.breed()["amplitude"][:, 1:].cpu().numpy()
    print("%d bred members against one control, %s norm, target %.4g, a rescale every %d steps: %d rescales in %d steps" % (
        info["bred"], args.norm, target, args.every, info["applied"], steps))
    print("  date               amplitude before the rescale (mean)   growth rate [1/day]: mean     min     max")
    for k, when in enumerate(model.breed_times()):
        if k % max(1, 36 // args.every) == 0 or k == len(growth) - 1:
            print("  %s   %35.4g   %25.3f %7.3f %7.3f" % (when.strftime("%Y-%m-%d %H:%M"), amplitude[k].mean(),
                                                        np.nanmean(growth[k]) if k else float("nan"),
                                                        np.nanmin(growth[k]) if k else float("nan"),
                                                        np.nanmax(growth[k]) if k else float("nan")))
    model.close()


if __name__ == "__main__":
    main()
