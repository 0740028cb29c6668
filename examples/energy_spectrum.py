#!/usr/bin/env python3
"""Kinetic-energy spectrum of a perturbed ensemble during its spin-up, recorded on the GPU at every step.

Every member gets the same boundary fields and a tiny random change of its grid-point temperature (as examples/climate_means.py).
The model records the rotational and the divergent kinetic-energy spectrum by total wavenumber at every step inside its own
multi-step calls, into a ring buffer in device memory (EnsembleModel.spectra_*): plain sums over the spectral coefficients the step
has just written, no transform.  After the run the script reads the series once and prints the time-mean spectrum of one level
(ensemble mean, rotational and divergent parts), its slope between total wavenumbers 10 and 25 (a least-squares line through
log E against log l), and by day the global-mean kinetic energy of that level with its spread over the members.

    python examples/energy_spectrum.py [--members 64] [--days 10] [--call-days 1] [--start 1982-01] [--noise 0.01] [--level 2]

API surface used: EnsembleModel.spectra_configure / spectra_info / spectra_times / spectra, run_checked (the reference's range check
of every step, recorded on the device), device_view + grid2spectral for the perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SLOPE_RANGE = (10, 25)  # total wavenumbers of the fitted line, both included


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])

    def between(lo, hi=None):
        def conv(text):
            v = int(text)
            if v < lo or (hi is not None and v > hi):
                raise argparse.ArgumentTypeError("must be at least %d" % lo if hi is None else "must be in %d ... %d" % (lo, hi))
            return v
        return conv

    p.add_argument("--members", type=between(2), default=64, help="ensemble size (the spread needs two)")
    p.add_argument("--days", type=between(1), default=10, help="days to simulate")
    p.add_argument("--call-days", type=between(1), default=1, help="days per device call")
    p.add_argument("--start", default="1982-01", help="first month, YYYY-MM")
    p.add_argument("--noise", type=float, default=0.01, help="standard deviation of the temperature perturbation [K]")
    p.add_argument("--level", type=between(0, 7), default=2, help="model level of the printed spectrum (0: top)")
    return p.parse_args(argv)


def slope(spectrum, lo=SLOPE_RANGE[0], hi=SLOPE_RANGE[1]):
    """Least-squares slope of log E(l) against log l over lo <= l <= hi."""
    l = np.arange(lo, hi + 1)
    return float(np.polyfit(np.log(l), np.log(np.asarray(spectrum)[lo:hi + 1]), 1)[0])


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

    samples = args.days * 36
    model.spectra_configure(["ke_rot_spectrum", "ke_div_spectrum"], 1, samples)  # every step
    left = args.days
    while left > 0:
        days = min(left, args.call_days)
        failed, _ = model.run_checked(36 * days)  # one device call; the samples inside it are taken by the device loop
        if (failed >= 0).any():
            raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())
        left -= days

    info = model.spectra_info()
    times = model.spectra_times()
    k = args.level
    rot = model.spectra("ke_rot_spectrum")[:, :, k]      # [M, samples, 32]
    div = model.spectra("ke_div_spectrum")[:, :, k]
    ke_mean = model.spectra("ke_mean")[:, :, k]          # [M, samples]: the sum over l of both parts
    rot_mean = rot.mean(dim=(0, 1)).cpu().numpy()        # time and ensemble mean
    div_mean = div.mean(dim=(0, 1)).cpu().numpy()
    print("%d members, %d samples every %d step(s) held of %d taken (%.2f MB on the device), level %d" % (
        args.members, info["held"], info["every"], info["taken"], info["capacity"] * args.members * 2 * 8 * 32 * 8 / 1e6, k))
    print("  time-mean kinetic-energy spectrum [J/kg], ensemble mean")
    print("     l    rotational     divergent         total")
    for l in range(1, 31):
        print("  %4d  %12.5e  %12.5e  %12.5e" % (l, rot_mean[l], div_mean[l], rot_mean[l] + div_mean[l]))
    print("  slope of log E against log l, l = %d ... %d: %.2f (rotational %.2f)" % (
        SLOPE_RANGE[0], SLOPE_RANGE[1], slope(rot_mean + div_mean), slope(rot_mean)))
    print("  day  valid             global-mean kinetic energy [J/kg]: ensemble mean, spread (std over the members)")
    mean = ke_mean.mean(dim=0).cpu().numpy()
    spread = ke_mean.std(dim=0, unbiased=True).cpu().numpy()
    for day in range(1, args.days + 1):
        j = 36 * day - 1
        print("  %3d  %s   %12.5e  %12.5e" % (day, times[j].strftime("%Y-%m-%d %H:%M"), mean[j], spread[j]))
    model.close()


if __name__ == "__main__":
    main()
