#!/usr/bin/env python3
"""Storm tracks as the literature defines them: the monthly variance of the 2-6-day band-passed 500 hPa height, on the GPU.

Every member gets the same boundary fields and a tiny random change of its grid-point temperature (as examples/climate_means.py).
The storm track is the variance of the band-passed Z500, not of Z500 itself; its companions are the transient eddy heat flux v'T'
at 850 hPa of the band-passed wind and temperature, and on the low-frequency side the variance of the 10-day low-passed height.
Separating time scales on the host means taping every six-hourly plane of every member.  The filter tape (EnsembleModel.filtape_*)
runs a recursive Butterworth filter per member and grid point on the device behind one step every six hours -- two planes of state
per second-order section instead of a window of samples -- and keeps only the monthly means of the filtered products: five planes
per member and month come back.  The first ten days run the filters and are counted in no window.

    python examples/bandpass_storm_tracks.py [--members 8] [--months 2]

API surface used: pyspeedy_amd.butterworth_sections, EnsembleModel.plev_configure, filtape_configure / filtape_info / filtape_times /
filtape_counts / filtape, run_checked, device_view + grid2spectral for the perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EVERY = 9     # model steps of 40 minutes: a sample every six hours
SPINUP = 40   # samples: ten days for the filters to forget the start
BAND, LOW = 0, 1


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])

    def at_least(n):
        def conv(text):
            v = int(text)
            if v < n:
                raise argparse.ArgumentTypeError("must be at least %d" % n)
            return v
        return conv

    p.add_argument("--members", type=at_least(1), default=8, help="ensemble size")
    p.add_argument("--months", type=at_least(1), default=2, help="months of 30 days to simulate from 1 January")
    return p.parse_args(argv)


def filters():
    """the 2-6-day band-pass (two sections) and the 10-day low-pass (one section) for six-hourly samples; periods in days"""
    import pyspeedy_amd
    return [pyspeedy_amd.butterworth_sections("bandpass", 2, (2.0, 6.0), 0.25), pyspeedy_amd.butterworth_sections("lowpass", 2, 10.0, 0.25)]


def entries():
    """levels of pressure-level names in hPa"""
    return [("z_plev", 500.0, BAND, "cov"),                          # the storm track: variance of the band-passed Z500
            ("v_plev", 850.0, BAND, "cov", "t_plev", 850.0),         # v'T' at 850 hPa
            ("u_plev", 250.0, BAND, "cov", "v_plev", 250.0),         # u'v' at 250 hPa
            ("z_plev", 500.0, LOW, "cov"),                           # second moment of the low-passed Z500 ...
            ("z_plev", 500.0, LOW, "mean")]                          # ... and its mean: variance = moment - mean^2


def main():
    args = parse_args()
    import torch
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel

    sp = pyspeedy_amd.ModSpectral(0)
    bc = np.load(os.path.join(os.path.dirname(pyspeedy_amd.__file__), "data", "example_bc.npz"))
    model = EnsembleModel(sp, args.members)
    model.init_sst_anom(args.months + 2)
    model.set_bc(bc, start_date=(1982, 1, 1, 0, 0))
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng(i).normal(0.0, 0.01, (96, 48, 8)).transpose(2, 1, 0) for i in range(args.members)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()

    model.plev_configure([850.0, 500.0, 250.0])
    model.filtape_configure(filters(), entries(), "month", args.months, sample_every=EVERY, spinup=SPINUP, dtype="float64")
    failed, _ = model.run_checked(36 * 30 * args.months)  # one device call for the whole run
    if (failed >= 0).any():
        raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())

    info = model.filtape_info
    counted, steps = model.filtape_counts()
    storm, vt, uv, low2, low1 = (model.filtape(k) for k in range(5))  # [members][months][48][96]
    low_var = low2 - low1 * low1
    lat = pyspeedy_amd.projection_weights(sp).lat
    print("%d members, %d windows held of %d closed, %d filtered planes, %d filter samples" % (
        args.members, info["held"], info["taken"], info["planes"], info["filter_samples"]))
    for w, when in enumerate(model.filtape_times()):
        zonal = storm[:, w].mean(dim=(0, 2)).sqrt().cpu().numpy()  # ensemble- and zonal-mean standard deviation by latitude
        j = int(np.argmax(zonal[24:])) + 24
        print("  window to %s: %d counted samples in %d steps; band-passed Z500 std peaks at %.1f N with %.1f m; "
              "v'T'(850) there %.2f K m/s, u'v'(250) %.2f m2/s2, low-passed Z500 std %.1f m" % (
                  when.strftime("%Y-%m-%d"), counted[w], steps[w], lat[j], zonal[j], float(vt[:, w, j].mean()), float(uv[:, w, j].mean()),
                  float(low_var[:, w, j].clamp(min=0).mean().sqrt())))
    model.close()


if __name__ == "__main__":
    main()
