#!/usr/bin/env python3
"""Monthly means, extremes and frost counts of a perturbed ensemble, accumulated on the GPU.

Every member gets the same boundary fields and a tiny random change of its grid-point temperature (as examples/climate_means.py).
The usual outputs of a climate run are per calendar month: the mean 500 hPa height and sea-level pressure, the strongest wind, the
coldest and warmest temperature, the number of six-hourly samples below freezing.  A calendar month is not a fixed number of steps,
so the window tape (EnsembleModel.wintape_*) closes its windows on the model's own calendar: it samples the state every 9 steps
(six hours) inside multi-step calls of `--call-days` days, accumulates on the device, and at every 00:00 of a day 1 writes the
month's results into a ring in device memory.  No call ends at a month boundary.  The first window starts with the run and the
last month is complete when the run ends at a month boundary; after the run the script reads the closed windows once and prints
them by month.

    python examples/monthly_climate.py [--members 16] [--months 2] [--call-days 5] [--start 1982-01] [--noise 0.01]

API surface used: EnsembleModel.plev_configure, wintape_configure / wintape_info / wintape_times / wintape_counts / wintape,
pyspeedy_amd.wintape_plan (the windows ahead, without a device), run_checked (the reference's range check of every step, recorded
on the device), device_view + grid2spectral for the perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SAMPLE_EVERY = 9   # model steps of 40 minutes: six hours
FREEZING = 273.15  # K
LEVELS_HPA = (500.0,)
ENTRIES = (("z_plev", "mean"), ("mslp", "mean"), ("wspd_grid", "max"), ("t_grid", "min"), ("t_grid", "max"),
           ("t_grid", "count_below", FREEZING))
MONTH_DAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


def days_of(year, month, months):
    """days of `months` calendar months from year-month, in the model's calendar (leap when year % 4 == 0)"""
    days = 0
    for _ in range(months):
        days += 29 if month == 2 and year % 4 == 0 else MONTH_DAYS[month - 1]
        month += 1
        if month > 12:
            year, month = year + 1, 1
    return days


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
    total_days = days_of(year, month, args.months)
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

    model.plev_configure(LEVELS_HPA)
    # the windows the run will close, from the library's own schedule (no device work): one per month, the ring's capacity
    ahead = pyspeedy_amd.wintape_plan((year, month, 1, 0, 0), 0, 36 * total_days, "month", sample_every=SAMPLE_EVERY)
    assert len(ahead) == args.months, ahead
    model.wintape_configure(ENTRIES, "month", len(ahead), sample_every=SAMPLE_EVERY, dtype="float64")
    left = total_days
    while left > 0:
        days = min(left, args.call_days)
        failed, _ = model.run_checked(36 * days)  # one device call, whatever month ends fall inside it
        if (failed >= 0).any():
            raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())
        left -= days

    info = model.wintape_info
    times = model.wintape_times()
    samples, steps = model.wintape_counts()
    z500 = model.wintape("z_plev", "mean")[:, :, 0]       # [M, months, lat, lon], m
    mslp = model.wintape("mslp", "mean") / 100.0          # hPa
    wind = model.wintape("wspd_grid", "max")              # [M, months, 8, lat, lon], m/s
    t_min = model.wintape("t_grid", "min")[:, :, -1]      # lowest model level, K
    t_max = model.wintape("t_grid", "max")[:, :, -1]
    frost = model.wintape("t_grid", "count_below")[:, :, -1]
    lat = torch.from_numpy(np.asarray(sp.table("radang"), dtype=np.float64)).to(z500.device)  # south to north
    w = torch.cos(lat)

    def globe(x):  # [M, months, lat, lon] -> [M, months]: area-weighted mean
        return (x.mean(dim=3) * w).sum(dim=2) / w.sum()

    g_z500, g_mslp, g_frost = (globe(x).cpu().numpy() for x in (z500, mslp, frost))
    g_wind = wind.amax(dim=(2, 3, 4)).cpu().numpy()
    g_tmin, g_tmax = t_min.amin(dim=(2, 3)).cpu().numpy(), t_max.amax(dim=(2, 3)).cpu().numpy()
    print("%d members, %d windows held of %d closed (window: %s, a sample every %d steps, %s)" % (
        args.members, info["held"], info["taken"], info["window"], info["sample_every"], info["dtype"]))
    print("  month ending       samples  steps   Z500 [m] mean +- spread   mslp [hPa]   max wind [m/s]   T lowest level [K] min / max"
          "   samples below %.2f K (area mean)" % FREEZING)
    for k, when in enumerate(times):
        print("  %s   %6d  %5d   %9.3f +- %8.2e   %10.3f   %14.2f   %12.2f / %6.2f   %10.3f" % (
            when.strftime("%Y-%m-%d %H:%M"), samples[k], steps[k], g_z500[:, k].mean(), g_z500[:, k].std(ddof=1), g_mslp[:, k].mean(),
            g_wind[:, k].max(), g_tmin[:, k].min(), g_tmax[:, k].max(), g_frost[:, k].mean()))
    model.close()


if __name__ == "__main__":
    main()
