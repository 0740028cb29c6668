#!/usr/bin/env python3
"""Monthly climate means of a perturbed ensemble, accumulated on the GPU while it runs.

Every member gets the same boundary fields and a tiny random change of its grid-point temperature.  The model samples
temperature and precipitation every `--every` steps inside its own multi-step calls (EnsembleModel.stats_*: nothing is copied to
the host while a month runs); each call ends at a month boundary, where the script reads the month's statistics and starts the
next averaging period.  It prints zonal means per month, ensemble mean and spread (the standard deviation over the members of
their monthly means), for a few latitudes, and -- from the 500 hPa height and the mean sea-level pressure the model interpolates
on the GPU at every sample (EnsembleModel.plev_configure) -- the time mean and standard deviation of Z500 and mslp.

    python examples/climate_means.py [--members 16] [--months 2] [--every 9] [--start 1982-01] [--noise 0.01]

API surface used: EnsembleModel.plev_configure, stats_configure / stats_mean / stats_var / stats_ensemble / stats_reset, run_checked (the reference's range
check of every step, recorded on the device), device_view + grid2spectral for the perturbation.
"""
import argparse
import calendar
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])

    def at_least(n):
        def conv(text):
            v = int(text)
            if v < n:
                raise argparse.ArgumentTypeError("must be at least %d" % n)
            return v
        return conv

    p.add_argument("--members", type=at_least(2), default=16, help="ensemble size (the spread needs two)")
    p.add_argument("--months", type=at_least(1), default=2, help="calendar months to simulate")
    p.add_argument("--every", type=at_least(1), default=9, help="model steps (40 min each) between two samples")
    p.add_argument("--start", default="1982-01", help="first month, YYYY-MM")
    p.add_argument("--noise", type=float, default=0.01, help="standard deviation of the temperature perturbation [K]")
    return p.parse_args(argv)


def main():
    args = parse()
    import torch
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel

    year, month = (int(v) for v in args.start.split("-"))
    sp = pyspeedy_amd.ModSpectral(0)
    bc = np.load(os.path.join(os.path.dirname(pyspeedy_amd.__file__), "data", "example_bc.npz"))
    model = EnsembleModel(sp, args.members)
    model.init_sst_anom(args.months + 2)
    model.set_bc(bc, start_date=(year, month, 1, 0, 0))
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng(i).normal(0.0, args.noise, (96, 48, 8)).transpose(2, 1, 0)
                      for i in range(args.members)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()

    lat = np.degrees(sp.table("radang"))  # Gaussian latitudes, south to north (j = 0 southernmost)
    rows = list(range(2, 48, 5))
    model.plev_configure([500.0])  # hPa: Z500 and the mean sea-level pressure are interpolated on the GPU at every sample
    model.stats_configure(["t_grid", "precnv", "precls", "z_plev", "mslp"], args.every, variance=True)
    for _ in range(args.months):
        steps = calendar.monthrange(year, month)[1] * 36
        failed, _ = model.run_checked(steps)  # one device call for the whole month
        if (failed >= 0).any():
            raise SystemExit("members %s left the accepted range in %04d-%02d" % (np.flatnonzero(failed >= 0).tolist(), year, month))
        # zonal means of every member's monthly mean, then mean and spread over the members
        t_zonal = model.stats_mean("t_grid").mean(dim=3)                                    # [M, lev, lat]
        p_zonal = (model.stats_mean("precnv") + model.stats_mean("precls")).mean(dim=2)     # [M, lat]
        t_ens, _ = model.stats_ensemble("t_grid")                                           # [lev, lat, lon], on the GPU
        print("%04d-%02d: %d samples, every %d steps; ensemble of %d" % (year, month, model.stats_samples, args.every, args.members))
        print("   lat   T lev 8 [K] (spread)   T lev 4 [K] (spread)   precnv + precls (spread)")
        tz = t_zonal.cpu().numpy()
        pz = p_zonal.cpu().numpy()
        te = t_ens.mean(dim=2).cpu().numpy()
        for j in rows:
            print("%6.1f  %8.2f (%8.2e)    %8.2f (%8.2e)    %8.4f (%8.2e)" % (
                lat[j], te[7, j], tz[:, 7, j].std(ddof=1), te[3, j], tz[:, 3, j].std(ddof=1), pz[:, j].mean(), pz[:, j].std(ddof=1)))
        # storm tracks and stationary waves: time mean and standard deviation of Z500 and mslp, and the members' spread of Z500
        z_mean, z_std, z_spread = model.stats_mean("z_plev"), model.stats_var("z_plev").sqrt(), model.stats_ensemble("z_plev")[1]
        p_mean, p_std = model.stats_mean("mslp") / 100.0, model.stats_var("mslp").sqrt() / 100.0
        print("   Z500 [m]: mean %.1f, time std %.1f (largest %.1f), ensemble spread of the mean %.2e;  mslp [hPa]: mean %.2f, time std %.2f"
              % (float(z_mean.mean()), float(z_std.mean()), float(z_std.max()), float(z_spread.mean()), float(p_mean.mean()), float(p_std.mean())))
        model.stats_reset()
        month += 1
        if month == 13:
            year, month = year + 1, 1
    model.close()


if __name__ == "__main__":
    main()
