#!/usr/bin/env python3
"""Six-hourly ensemble mean and spread of Z500 and mean sea-level pressure, reduced over the members on the GPU.

Every member gets the same boundary fields and a tiny random change of its grid-point temperature (as
examples/six_hourly_series.py).  Where that example records every member's field on the tape and reduces afterwards, this one
records the reduction itself (EnsembleModel.enstape_*): after every 9 steps (6 hours) the device loop folds the members' 500 hPa
height and mean sea-level pressure into an ensemble mean and a sum of squared deviations, per grid point, inside the multi-step
call.  The ring holds two planes per sample and member group whatever the ensemble size, so a 1024-member ensemble records a year
in the memory the tape needs for a day.  After the run the script reads mean and standard deviation once and prints, per sample,
the area-weighted spread of both fields.

    python examples/ensemble_spread_series.py [--members 64] [--days 30] [--call-days 5] [--start 1982-01] [--noise 0.01]
                                              [--block-members 0]

API surface used: EnsembleModel.plev_configure, enstape_configure / enstape_info / enstape_times / enstape, run_checked (the
reference's range check of every step, recorded on the device), set_option("block_members") for large ensembles, device_view +
grid2spectral for the perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EVERY = 9  # model steps of 40 minutes: 6 hours
NAMES = ("z_plev", "mslp")


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])

    def at_least(n):
        def conv(text):
            v = int(text)
            if v < n:
                raise argparse.ArgumentTypeError("must be at least %d" % n)
            return v
        return conv

    p.add_argument("--members", type=at_least(2), default=64, help="ensemble size (the spread needs two)")
    p.add_argument("--days", type=at_least(1), default=30, help="days to simulate")
    p.add_argument("--call-days", type=at_least(1), default=5, help="days per device call")
    p.add_argument("--start", default="1982-01", help="first month, YYYY-MM")
    p.add_argument("--noise", type=float, default=0.01, help="standard deviation of the temperature perturbation [K]")
    p.add_argument("--block-members", type=at_least(0), default=0,
                   help="step large ensembles in rounds of this many members per group (0: all members at once)")
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
    if args.block_members:
        model.set_option("block_members", args.block_members)
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng(i).normal(0.0, args.noise, (96, 48, 8)).transpose(2, 1, 0)
                      for i in range(args.members)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()

    samples = args.days * 36 // EVERY
    model.plev_configure([500.0])  # hPa
    model.enstape_configure(NAMES, EVERY, samples)
    left = args.days
    while left > 0:
        days = min(left, args.call_days)
        failed, _ = model.run_checked(36 * days)  # one device call; the samples inside it are reduced by the device loop
        if (failed >= 0).any():
            raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())
        left -= days

    info = model.enstape_info
    times = model.enstape_times()
    z_mean, z_std = model.enstape("z_plev")     # [samples, 1, lat, lon]
    p_mean, p_std = model.enstape("mslp")       # [samples, lat, lon], Pa
    lat = torch.from_numpy(np.asarray(sp.table("radang"), dtype=np.float64)).to(z_std.device)  # south to north
    w = torch.cos(lat)
    north = (torch.rad2deg(lat) >= 30.0).double() * w

    def area(x, weights):  # [samples, lat, lon] -> [samples]
        return ((x.mean(dim=2) * weights).sum(dim=1) / weights.sum()).cpu().numpy()

    z_globe, z_north = area(z_std[:, 0], w), area(z_std[:, 0], north)
    p_globe = area(p_std / 100.0, w)
    z_bar = area(z_mean[:, 0], w)
    print("%d members, %d samples every %d steps held of %d taken (%.1f MB on the device; a float32 tape of the same names: %.1f MB)" % (
        info["members"], info["held"], info["every"], info["taken"], info["capacity"] * 4 * 2 * 4608 * 16 / 1e6,
        info["capacity"] * info["members"] * 2 * 4608 * 4 / 1e6))
    print("  lead [h]  valid             Z500 mean [m]   Z500 spread [m] globe / north of 30N   mslp spread [hPa]")
    stride = max(1, len(times) // 40)
    for k in range(0, len(times), stride):
        print("  %7d   %s   %10.3f      %10.3e / %10.3e              %10.3e" % (
            6 * (k + 1), times[k].strftime("%Y-%m-%d %H:%M"), z_bar[k], z_globe[k], z_north[k], p_globe[k]))
    model.close()


if __name__ == "__main__":
    main()
