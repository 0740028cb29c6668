#!/usr/bin/env python3
"""Probability maps of a forecast week: the distribution over the members at every grid point, formed inside the device call.

A perturbed ensemble runs for a week in one run_checked() call.  Once a day the quantile tape leaves, per grid point:
the share of the members whose convective precipitation rate exceeds 1 mm/day, the 10 / 50 / 90 % quantiles of the 500 hPa height,
and the lowest member's temperature at the lowest model level.  No member's plane leaves the device: the host reads five maps per
day, whatever the size of the ensemble.

    python examples/probability_maps.py [--members 20] [--days 7] [--every 36] [--seed 0]

API surface used: EnsembleModel.set_bc / run / run_checked, plev_configure, qtape_configure / qtape / qtape_steps / qtape_times /
qtape_entries / qtape_info.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPINUP = 36                     # a day, so that the members have diverged and convection has begun
STEPS_PER_DAY = 36              # 2400 s steps
MM_PER_DAY = 1000.0 / 86400.0   # 1 mm/day as a rate in g/(m^2 s), the unit of precnv
LEVELS_HPA = (500.0,)


def entries():
    """(name, level, op[, param]) of the quantile tape, in the order the maps are read in"""
    return [("precnv", 0, "prob_above", MM_PER_DAY),
            ("z_plev", 0, "quantile", 0.1), ("z_plev", 0, "quantile", 0.5), ("z_plev", 0, "quantile", 0.9),
            ("t_grid", 7, "min")]


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--members", type=int, default=20, help="members of the ensemble, 2 ... 64 (default 20)")
    ap.add_argument("--days", type=int, default=7, help="days of forecast (default 7)")
    ap.add_argument("--every", type=int, default=STEPS_PER_DAY, help="steps between two sets of maps (default 36: daily)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if not 2 <= args.members <= 64:
        ap.error("--members must be 2 ... 64")
    if args.days < 1:
        ap.error("--days must be at least 1")
    if args.every < 1:
        ap.error("--every must be at least 1")
    return args


def perturb(model, seed):
    """a different temperature for every member: factors 1 + 2e-4 N(0, 1) on the spectral coefficients, the zonal means kept real"""
    for i in range(model.nmembers):
        f = 1.0 + 2e-4 * np.random.default_rng([seed, i]).standard_normal((31, 32, 8, 1))
        f[0] = 1.0
        model.set("t", model.get("t", i) * f, i)


def main():
    args = parse()
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel

    sp = pyspeedy_amd.ModSpectral(0)
    bc = np.load(os.path.join(os.path.dirname(pyspeedy_amd.__file__), "data", "example_bc.npz"))
    model = EnsembleModel(sp, args.members)
    model.set_bc(bc)
    perturb(model, args.seed)
    model.run(SPINUP)
    model.plev_configure(LEVELS_HPA)
    steps = args.days * STEPS_PER_DAY
    model.qtape_configure(entries(), np.ones(args.members, dtype=np.int32), args.every, capacity=max(steps // args.every + 1, 1))
    failed, _ = model.run_checked(steps)
    if (failed >= 0).any():
        raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())
    info = model.qtape_info()
    times = model.qtape_times()
    maps = [model.qtape(k).cpu().numpy() for k in range(len(model.qtape_entries))]  # each [events][48][96]
    model.close()

    wet, z10, z50, z90, tmin = maps
    assert (z10 <= z50).all() and (z50 <= z90).all()
    print("%d members, maps every %d steps: %d events" % (info["members"], info["every"], info["held"]))
    print("  date               P(precnv > 1 mm/day): points > 0 / > 0.5 / = 1   Z500 90 % - 10 % [m]: mean / max     coldest member T [K]: min")
    for t, when in enumerate(times):
        spread = z90[t] - z10[t]
        print("  %s   %22d / %5d / %5d   %30.2f / %6.2f   %26.2f" % (
            when.strftime("%Y-%m-%d %H:%M"), int((wet[t] > 0).sum()), int((wet[t] > 0.5).sum()), int((wet[t] == 1.0).sum()),
            float(spread.mean()), float(spread.max()), float(tmin[t].min())))


if __name__ == "__main__":
    main()
