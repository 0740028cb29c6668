#!/usr/bin/env python3
"""A perfect-model assimilation experiment (OSSE) with the ensemble square-root filter inside one multi-day device call.

A one-member nature run records a handful of station and box observations through the projection tape, every --every steps.
Seeded Gaussian noise of the stated error is added on the host.  An ensemble whose members start from perturbed temperatures
then assimilates them, every --every steps, inside ONE run_checked() call of --steps steps: the observation operators are the
same weight maps, the analysis is the serial ensemble square-root filter of DESIGN section 4l, computed and applied on the device
between the steps.  Member 0 of the ensemble is left out of the analysis (mask 0) and shows what the perturbed start does without
observations.  The innovation statistics come from the filter's ring: for a consistent filter the innovations have zero mean and
the variance s + R that the ring's prior variance s and the error variance R predict.

    python examples/osse_ensrf.py [--members 20] [--steps 360] [--every 9] [--inflation 1.02] [--seed 0]

API surface used: pyspeedy_amd.projection_weights, EnsembleModel.projtape_configure / projtape / projtape_steps for the nature
run, assim_configure / assim_observations / assim / assim_steps / assim_info / assim_compute for the ensemble, run_checked.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STATIONS = ((10.0, 50.0), (255.0, 40.0), (140.0, -35.0))  # (lon, lat)
BOX = (150.0, -150.0, -20.0, 20.0)                         # across the date line
# (name, level, pattern): lowest-level temperature at the stations, a mid-level temperature and an upper wind over the box, and the
# box's surface pressure; SIGMA: the standard deviation of each observation's error, in the export's units (K, K, K, K, m/s, Pa)
ENTRIES = (("t_grid", 7, 0), ("t_grid", 7, 1), ("t_grid", 7, 2), ("t_grid", 4, 3), ("u_grid", 2, 3), ("ps_grid", 0, 3))
SIGMA = (0.5, 0.5, 0.5, 0.3, 1.0, 50.0)
SPINUP = 72  # steps both runs take before the first observation


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])

    def between(lo, hi=None):
        def conv(text):
            v = int(text)
            if v < lo or (hi is not None and v > hi):
                raise argparse.ArgumentTypeError("must be at least %d%s" % (lo, "" if hi is None else " and at most %d" % hi))
            return v
        return conv

    def inflation(text):
        v = float(text)
        if not (np.isfinite(v) and v >= 1.0):
            raise argparse.ArgumentTypeError("must be a finite number >= 1")
        return v

    p.add_argument("--members", type=between(2, 63), default=20, help="members that assimilate (one more runs freely beside them)")
    p.add_argument("--steps", type=between(1, 4096), default=360, help="steps of the assimilating call (360: ten days)")
    p.add_argument("--every", type=between(1), default=9, help="model steps of 40 minutes between two analyses (9: six hours)")
    p.add_argument("--inflation", type=inflation, default=1.02, help="multiplicative inflation of the prior perturbations")
    p.add_argument("--seed", type=int, default=0, help="seed of the observation noise and of the initial perturbations")
    return p.parse_args(argv)


def mask_of(members):
    """member 0 runs freely, the `members` others assimilate"""
    mask = np.ones(members + 1, dtype=np.int32)
    mask[0] = 0
    return mask


def weight_maps(pw):
    return np.stack([pw.point(*s) for s in STATIONS] + [pw.box(*BOX)])


def perturb(model, seed, std=1.0):
    """a different temperature per member: grid-point noise of `std` K, through the model's own transforms"""
    import torch
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng([seed, i]).normal(0.0, std, (96, 48, 8)).transpose(2, 1, 0) for i in range(model.nmembers)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()


def main():
    args = parse()
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel

    sp = pyspeedy_amd.ModSpectral(0)
    bc = np.load(os.path.join(os.path.dirname(pyspeedy_amd.__file__), "data", "example_bc.npz"))
    maps = weight_maps(pyspeedy_amd.projection_weights(sp))
    sigma = np.asarray(SIGMA)

    # the nature run: the truth's values of every entry at the analysis steps
    nature = EnsembleModel(sp, 1)
    nature.set_bc(bc)
    nature.run(SPINUP)
    nature.projtape_configure(maps, ENTRIES, args.every, max(args.steps // args.every + 1, 1))
    nature.run(args.steps)
    truth = nature.projtape()[0].cpu().numpy()  # [T][E]
    stamps = nature.projtape_steps()
    nature.close()
    yo = truth + sigma * np.random.default_rng([args.seed, 1 << 20]).standard_normal(truth.shape)

    # the ensemble: one call, the analyses on the device between its steps
    model = EnsembleModel(sp, args.members + 1)
    model.set_bc(bc)
    perturb(model, args.seed)
    model.run(SPINUP)
    model.assim_configure(maps, ENTRIES, mask_of(args.members), args.every, capacity=len(stamps), inflation=args.inflation)
    model.assim_observations(stamps, yo, sigma ** 2)
    failed, _ = model.run_checked(args.steps)
    if (failed >= 0).any():
        raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())
    info, ring = model.assim_info(), {k: v.cpu().numpy() for k, v in model.assim().items()}
    final = model.assim_compute().cpu().numpy()  # [E][members] at the end of the call
    model.close()

    print("%d members, %d entries, an analysis every %d steps: %d executed, %d skipped in %d steps (inflation %.3g)" % (
        info["members"], info["entries"], info["every"], info["applied"], info["skipped"], args.steps, args.inflation))
    print("  entry                 sigma_o   mean innovation   rms innovation   predicted sqrt(s + R)   prior spread first -> last   used")
    for e, (name, level, pattern) in enumerate(ENTRIES):
        v, s = ring["innovation"][:, e], ring["variance"][:, e]
        print("  %-10s %d map %d   %8.3g   %15.4g   %14.4g   %21.4g   %12.4g -> %-10.4g   %d / %d" % (
            name, level, pattern, sigma[e], v.mean(), np.sqrt((v ** 2).mean()), np.sqrt((s + sigma[e] ** 2).mean()), np.sqrt(s[0]),
            np.sqrt(s[-1]), int(ring["used"][:, e].sum()), len(v)))
    err = np.abs(final.mean(axis=1) - truth[-1]) if stamps[-1] == SPINUP + args.steps else None
    if err is not None:
        print("  |analysis mean - truth| at the last step, in sigma_o:", " ".join("%.2f" % x for x in err / sigma))


if __name__ == "__main__":
    main()
