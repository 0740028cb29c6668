#!/usr/bin/env python3
"""Leading Lyapunov exponents of a SPEEDY trajectory from orthonormalised breeding inside one multi-day device call.

Member 0 is the control; every other member starts from it with a small random temperature perturbation and runs a first day
freely; the mean amplitude the perturbations have then is the target.  From there on, every --every steps (9 steps of 40
minutes: six hours) the perturbations are orthonormalised on the device, between the steps of ONE run_checked() call: the
Gram-Schmidt cycle in the chosen norm, member 1 first.  Member j keeps the part of its grown perturbation that is orthogonal to
those of the members before it, rescaled to the target; the ring keeps the size R_jj of that part, and the time mean of
ln(R_jj / target) over the cycle length is the j-th local Lyapunov exponent.  Plain breeding runs beside it from the same start:
its members collapse onto the leading bred vector, which the bred-vector dimension of the Gram matrix shows (1: one direction,
members - 1: all independent).

    python examples/lyapunov_spectrum.py [--members 8] [--days 30] [--every 9] [--norm total_energy] [--noise 0.01]

API surface used: pyspeedy_amd.breed_weights, EnsembleModel.breed_configure(orthogonalize=True) / breed_amplitude / breed_gram /
breed_exponents / breed_info, run_checked, device_view + grid2spectral for the perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NORMS = ("kinetic_energy", "total_energy", "t_rms")


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])

    def between(lo, hi=None):
        def conv(text):
            v = int(text)
            if v < lo or (hi is not None and v > hi):
                raise argparse.ArgumentTypeError("must be at least %d%s" % (lo, "" if hi is None else " and at most %d" % hi))
            return v
        return conv

    p.add_argument("--members", type=between(2, 65), default=8, help="ensemble size: one control and members - 1 bred members (a family of at most 64)")
    p.add_argument("--days", type=between(1), default=30, help="days to simulate, as one device call")
    p.add_argument("--every", type=between(1), default=9, help="model steps of 40 minutes between two orthonormalisations (9: six hours)")
    p.add_argument("--norm", choices=NORMS, default="total_energy", help="the inner product")
    p.add_argument("--noise", type=float, default=0.01, help="standard deviation of the initial temperature perturbation [K]")
    return p.parse_args(argv)


def control_of(members):
    """member 0 is the control of all others"""
    control = np.zeros(members, dtype=np.int32)
    control[0] = -1
    return control


def dimension(gram):
    """The bred-vector dimension (sum sigma)^2 / sum sigma^2 of the perturbations with Gram matrix `gram`, sigma the singular values
    of the perturbations scaled to unit length: 1 if all point the same way, their number if they are orthogonal."""
    g = np.asarray(gram, dtype=np.float64)
    d = np.sqrt(np.diag(g))
    sigma = np.sqrt(np.clip(np.linalg.eigvalsh(g / np.outer(d, d)), 0.0, None))
    return float(sigma.sum() ** 2 / (sigma ** 2).sum())


def main():
    args = parse()
    import torch
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel

    sp = pyspeedy_amd.ModSpectral(0)
    bc = np.load(os.path.join(os.path.dirname(pyspeedy_amd.__file__), "data", "example_bc.npz"))
    steps = 36 * args.days
    events = max(steps // args.every, 1)
    weights = pyspeedy_amd.breed_weights(args.norm)
    control = control_of(args.members)
    result = {}
    for orthogonalize in (True, False):
        model = EnsembleModel(sp, args.members)
        model.set_bc(bc)
        model.spectral2grid()
        t_grid = model.device_view("t_grid")
        noise = np.stack([np.zeros((8, 48, 96)) if i == 0 else
                          np.random.default_rng(i).normal(0.0, args.noise, (96, 48, 8)).transpose(2, 1, 0) for i in range(args.members)])
        t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
        model.grid2spectral()
        model.run(36)  # a first day without rescaling; the mean amplitude after it is the target
        model.breed_configure(control, 1.0, args.every, weights=weights, capacity=events, in_loop=False)
        target = float(model.breed_amplitude()[1:].mean())
        model.breed_configure(control, target, args.every, weights=weights, capacity=events, orthogonalize=orthogonalize)
        failed, _ = model.run_checked(steps)  # one device call: every step checked, every cycle orthonormalised on the device
        if (failed >= 0).any():
            raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())
        result[orthogonalize] = dict(exponents=model.breed_exponents()[1:], info=model.breed_info(), target=target)
        # one more cycle without a rescale at its end: the Gram matrix of what the perturbations have grown into
        model.breed_configure(control, target, args.every, weights=weights, capacity=1, in_loop=False)
        model.run(args.every)
        result[orthogonalize]["gram"] = model.breed_gram()[1:, 1:].cpu().numpy()
        model.close()

    info = result[True]["info"]
    print("%d bred members against one control, %s norm, target %.4g, orthonormalised every %d steps: %d times in %d steps" % (
        info["bred"], args.norm, result[True]["target"], args.every, info["applied"], steps))
    print("  Lyapunov exponents [1/day], descending:", " ".join("%.3f" % v for v in np.sort(result[True]["exponents"])[::-1]))
    print("  plain breeding, growth rates [1/day]:  ", " ".join("%.3f" % v for v in np.sort(result[False]["exponents"])[::-1]))
    print("  bred-vector dimension of the %d perturbations: %.2f orthonormalised, %.2f with plain breeding" % (
        info["bred"], dimension(result[True]["gram"]), dimension(result[False]["gram"])))


if __name__ == "__main__":
    main()
