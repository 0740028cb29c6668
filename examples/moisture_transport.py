#!/usr/bin/env python3
"""Vertical velocity, column water vapour and the moisture transport of a perturbed ensemble, recorded on the GPU.

Every member gets the same boundary fields and a tiny random change of its grid-point temperature (as examples/climate_means.py).
Three recorders take derived fields inside the model's own multi-step calls, and no output time ends one:

  - the tape: omega at 500 hPa (the model's own continuity equation, interpolated to the pressure level) and the column water
    vapour every 9 steps (6 hours), as float32;
  - the projection tape: the area mean of the column water vapour over a box (the tropical west Pacific), one number per member
    and sample;
  - the window tape: monthly means of the two components of the vertically integrated moisture transport.

After the run the script reads each once and prints the ensemble-mean series of the box mean with its spread, the strongest ascent
and descent at 500 hPa, and the zonal means of the monthly transport.

    python examples/moisture_transport.py [--members 8] [--days 30] [--call-days 5] [--start 1982-01] [--noise 0.01]

API surface used: EnsembleModel.plev_configure, tape_configure / tape / tape_times, pyspeedy_amd.projection_weights,
projtape_configure / projtape, wintape_configure / wintape / wintape_times, run_checked; the names are those of
EnsembleModel.DERIVED_VARIABLES (derived() gives the same fields between calls).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EVERY = 9  # model steps of 40 minutes: 6 hours
BOX = (120.0, 180.0, -10.0, 10.0)  # lon0, lon1, lat0, lat1


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--members", type=int, default=8, help="ensemble size")
    p.add_argument("--days", type=int, default=30, help="days to simulate")
    p.add_argument("--call-days", type=int, default=5, help="days per device call")
    p.add_argument("--start", default="1982-01", help="first month, YYYY-MM")
    p.add_argument("--noise", type=float, default=0.01, help="standard deviation of the temperature perturbation [K]")
    args = p.parse_args(argv)
    if args.members < 1 or args.days < 1 or args.call_days < 1:
        p.error("--members, --days and --call-days must be at least 1")
    return args


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
    model.tape_configure(["omega_plev", "tcwv"], EVERY, samples, dtype="float32")
    box = pyspeedy_amd.projection_weights(sp).box(*BOX)
    model.projtape_configure(box[None], [("tcwv", 0, 0)], EVERY, samples)
    model.wintape_configure([("ivt_u", "mean"), ("ivt_v", "mean")], "month", args.days // 28 + 2, sample_every=EVERY)
    left = args.days
    while left > 0:
        days = min(left, args.call_days)
        failed, _ = model.run_checked(36 * days)  # one device call; the samples inside it are taken by the device loop
        if (failed >= 0).any():
            raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())
        left -= days

    times = model.tape_times()
    omega = model.tape("omega_plev")[:, :, 0].double()   # [M, samples, lat, lon], Pa/s
    series = model.projtape()[:, :, 0].cpu().numpy()     # [M, samples], kg/m^2
    tcwv = model.tape("tcwv").double()
    print("%d members, %d samples every %d steps; column water vapour %.1f ... %.1f kg/m^2" % (
        args.members, len(times), EVERY, float(tcwv.min()), float(tcwv.max())))
    print("  valid             box-mean tcwv [kg/m^2] mean (spread)   omega500 [Pa/s] strongest ascent / descent (ensemble mean)")
    up = omega.amin(dim=(2, 3)).mean(dim=0).cpu().numpy()
    down = omega.amax(dim=(2, 3)).mean(dim=0).cpu().numpy()
    stride = max(1, len(times) // 30)
    for k in range(0, len(times), stride):
        spread = series[:, k].std(ddof=1) if args.members > 1 else 0.0
        print("  %s   %8.3f (%.2e)                      %8.3f / %7.3f" % (
            times[k].strftime("%Y-%m-%d %H:%M"), series[:, k].mean(), spread, up[k], down[k]))
    months = model.wintape_times()
    if months:
        lat = np.rad2deg(np.asarray(sp.table("radang"), dtype=np.float64))
        ivt_u = model.wintape("ivt_u", "mean").double().mean(dim=(0, 3)).cpu().numpy()  # [months, lat]
        ivt_v = model.wintape("ivt_v", "mean").double().mean(dim=(0, 3)).cpu().numpy()
        for j, when in enumerate(months):
            print("month ending %s: zonal-mean moisture transport [kg/(m s)], eastward / northward" % when.strftime("%Y-%m-%d"))
            for row in range(0, 48, 6):
                print("  %6.1f   %8.2f / %7.2f" % (lat[row], ivt_u[j, row], ivt_v[j, row]))
    else:
        print("no month ended inside the run: the window tape holds no window yet")
    model.close()


if __name__ == "__main__":
    main()
