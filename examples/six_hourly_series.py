#!/usr/bin/env python3
"""Six-hourly series of Z500, mean sea-level pressure and precipitation of a perturbed ensemble, recorded on the GPU.

Every member gets the same boundary fields and a tiny random change of its grid-point temperature (as examples/climate_means.py).
The model records the 500 hPa height, the mean sea-level pressure and the two precipitation fields every 9 steps (6 hours) inside
its own multi-step calls, into a ring buffer in device memory (EnsembleModel.tape_*): the calls are `--call-days` days long and no
output time ends one.  After the run the script reads the series once and prints, by lead time, the ensemble spread of Z500 (the
standard deviation over the members, averaged over the globe with area weights and over the northern extratropics), and the
ensemble-mean precipitation.

    python examples/six_hourly_series.py [--members 16] [--days 30] [--call-days 1] [--start 1982-01] [--noise 0.01] [--dtype float32]

API surface used: EnsembleModel.plev_configure, tape_configure / tape_info / tape_times / tape, run_checked (the reference's range
check of every step, recorded on the device), device_view + grid2spectral for the perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EVERY = 9  # model steps of 40 minutes: 6 hours


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
    p.add_argument("--days", type=at_least(1), default=30, help="days to simulate")
    p.add_argument("--call-days", type=at_least(1), default=1, help="days per device call")
    p.add_argument("--start", default="1982-01", help="first month, YYYY-MM")
    p.add_argument("--noise", type=float, default=0.01, help="standard deviation of the temperature perturbation [K]")
    p.add_argument("--dtype", choices=("float32", "float64"), default="float32", help="storage of the tape")
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

    samples = args.days * 36 // EVERY
    model.plev_configure([500.0])  # hPa
    model.tape_configure(["z_plev", "mslp", "precnv", "precls"], EVERY, samples, dtype=args.dtype)
    left = args.days
    while left > 0:
        days = min(left, args.call_days)
        failed, _ = model.run_checked(36 * days)  # one device call; the samples inside it are taken by the device loop
        if (failed >= 0).any():
            raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())
        left -= days

    info = model.tape_info
    times = model.tape_times()
    z500 = model.tape("z_plev")[:, :, 0].double()                       # [M, samples, lat, lon]
    mslp = model.tape("mslp").double() / 100.0                          # hPa
    precip = (model.tape("precnv") + model.tape("precls")).double()     # as the column physics stores them
    lat = torch.from_numpy(np.asarray(sp.table("radang"), dtype=np.float64)).to(z500.device)  # south to north
    w = torch.cos(lat)
    north = (torch.rad2deg(lat) >= 30.0).double() * w
    spread = z500.std(dim=0, unbiased=True).mean(dim=2)                 # [samples, lat]: zonal mean of the members' spread
    s_globe = (spread * w).sum(dim=1) / w.sum()
    s_north = (spread * north).sum(dim=1) / north.sum()
    p_mean = (precip.mean(dim=0).mean(dim=2) * w).sum(dim=1) / w.sum()
    m_spread = (mslp.std(dim=0, unbiased=True).mean(dim=2) * w).sum(dim=1) / w.sum()
    print("%d members, %d samples every %d steps held of %d taken (%s, %.1f MB on the device)" % (
        args.members, info["held"], info["every"], info["taken"], info["dtype"],
        info["capacity"] * args.members * 4 * 4608 * (4 if info["dtype"] == "float32" else 8) / 1e6))
    print("  lead [h]  valid             Z500 spread [m] globe / north of 30N   mslp spread [hPa]   precipitation (ensemble mean)")
    s_globe, s_north, p_mean, m_spread = (x.cpu().numpy() for x in (s_globe, s_north, p_mean, m_spread))
    stride = max(1, len(times) // 40)
    for k in range(0, len(times), stride):
        print("  %7d   %s   %10.3e / %10.3e              %10.3e          %8.4f" % (
            6 * (k + 1), times[k].strftime("%Y-%m-%d %H:%M"), s_globe[k], s_north[k], m_spread[k], p_mean[k]))
    model.close()


if __name__ == "__main__":
    main()
