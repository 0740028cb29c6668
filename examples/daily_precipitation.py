#!/usr/bin/env python3
"""Daily precipitation totals and daily-mean radiation of a perturbed ensemble, accumulated on the GPU.

Every member gets the same boundary fields and a tiny random change of its grid-point temperature (as examples/climate_means.py).
Precipitation is intermittent: a value every few steps says little about what fell in a day.  The accumulation tape
(EnsembleModel.acctape_*) adds up what the column physics stores on EVERY step and closes a window every 36 steps (one day) into a
ring in device memory, inside multi-step calls of `--call-days` days: the sum of convective and large-scale precipitation, the
strongest convective rain of the day, and the daily means of outgoing longwave and net shortwave radiation at the top.  After the
run the script reads the windows once and prints the area-weighted daily totals by day.

The library keeps the registry's own units: precipitation is a rate in g/(m^2 s), valid for the 2400 s of its step.  The script turns
the sum over a day's steps into mm/day: sum x 2400 s x 1e-3 (kg per g; 1 kg/m^2 of water is 1 mm).

    python examples/daily_precipitation.py [--members 16] [--days 10] [--call-days 5] [--start 1982-01] [--noise 0.01]

API surface used: EnsembleModel.acctape_configure / acctape_info / acctape_times / acctape_counts / acctape, run_checked (the
reference's range check of every step, recorded on the device), device_view + grid2spectral for the perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EVERY = 36             # model steps of 40 minutes: one day
STEP_SECONDS = 2400.0  # what a stored precipitation rate is valid for
ENTRIES = (("precnv", "sum"), ("precls", "sum"), ("precnv", "max"), ("olr", "mean"), ("tsr", "mean"))


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
    p.add_argument("--days", type=at_least(1), default=10, help="days to simulate")
    p.add_argument("--call-days", type=at_least(1), default=5, help="days per device call")
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
    model.init_sst_anom(args.days // 28 + 3)
    model.set_bc(bc, start_date=(year, month, 1, 0, 0))
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng(i).normal(0.0, args.noise, (96, 48, 8)).transpose(2, 1, 0)
                      for i in range(args.members)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()

    model.acctape_configure(ENTRIES, EVERY, args.days, dtype="float64")
    left = args.days
    while left > 0:
        days = min(left, args.call_days)
        failed, _ = model.run_checked(36 * days)  # one device call; every step of it adds to the open window on the device
        if (failed >= 0).any():
            raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())
        left -= days

    info = model.acctape_info
    times, counts = model.acctape_times(), model.acctape_counts()
    to_mm = STEP_SECONDS * 1.0e-3  # g/(m^2 s) summed over steps -> mm
    total = (model.acctape("precnv", "sum") + model.acctape("precls", "sum")) * to_mm   # [M, days, lat, lon], mm/day
    conv = model.acctape("precnv", "sum") * to_mm
    peak = model.acctape("precnv", "max") * (86400.0 * 1.0e-3)                          # strongest step, as a rate in mm/day
    olr, tsr = model.acctape("olr", "mean"), model.acctape("tsr", "mean")              # W/m^2
    lat = torch.from_numpy(np.asarray(sp.table("radang"), dtype=np.float64)).to(total.device)  # south to north
    w = torch.cos(lat)

    def globe(x):  # [M, days, lat, lon] -> [M, days]: area-weighted mean
        return (x.mean(dim=3) * w).sum(dim=2) / w.sum()

    g_total, g_conv, g_olr, g_tsr = (globe(x).cpu().numpy() for x in (total, conv, olr, tsr))
    g_peak = peak.amax(dim=(2, 3)).cpu().numpy()
    print("%d members, %d windows of %d steps held of %d closed (%s)" % (
        args.members, info["held"], info["every"], info["taken"], info["dtype"]))
    print("  day ending         steps   precipitation [mm/day] mean +- spread   convective   peak conv. rate   OLR [W/m2]   TSR [W/m2]")
    for k, when in enumerate(times):
        print("  %s   %5d   %10.4f +- %8.2e              %10.4f   %12.2f   %10.3f   %10.3f" % (
            when.strftime("%Y-%m-%d %H:%M"), counts[k], g_total[:, k].mean(), g_total[:, k].std(ddof=1), g_conv[:, k].mean(),
            g_peak[:, k].max(), g_olr[:, k].mean(), g_tsr[:, k].mean()))
    model.close()


if __name__ == "__main__":
    main()
