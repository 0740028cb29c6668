#!/usr/bin/env python3
"""The track of the deepest North-Atlantic low of every member of a perturbed ensemble, followed on the GPU.

Every member gets the same boundary fields and a tiny random change of its grid-point temperature (as examples/climate_means.py).
"How deep is the low, and where is it?" is an argmin over a region, and a track is that argmin followed from sample to sample: no
weight map of the projection tape expresses it, and taping whole planes of sea-level pressure to take the argmin on the host is
18 KB per member and sample.  The track tape (EnsembleModel.tracktape_*) finds the minimum of mslp over a North-Atlantic box on the
device behind one step every six hours inside a single multi-day call, and -- with radius 2 -- looks from the second sample on only
within two grid points of where it found the low last, so that it stays with ONE low while a deeper one forms elsewhere in the
box.  32 bytes per member and sample come back: the pressure, the grid point and two sub-grid offsets, which tracktape_lonlat turns
into degrees.  A second entry with radius 0 shows the deepest point of the box at each sample, for comparison.

    python examples/storm_track.py [--members 8] [--days 5]

API surface used: pyspeedy_amd.projection_weights (box), EnsembleModel.plev_configure, tracktape_configure / tracktape_info /
tracktape_times / tracktape / tracktape_positions / tracktape_lonlat, run_checked, device_view + grid2spectral for the perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EVERY = 9  # model steps of 40 minutes: a sample every six hours
RADIUS = 2  # grid points (7.5 degrees) a low may move between two samples
BOX = (280.0, 350.0, 30.0, 70.0)  # 80 W ... 10 W, 30 N ... 70 N


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])

    def at_least(n):
        def conv(text):
            v = int(text)
            if v < n:
                raise argparse.ArgumentTypeError("must be at least %d" % n)
            return v
        return conv

    p.add_argument("--members", type=at_least(1), default=8, help="ensemble size")
    p.add_argument("--days", type=at_least(1), default=5, help="days to simulate: four samples a day")
    return p.parse_args(argv)


def main():
    args = parse()
    import torch
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel

    sp = pyspeedy_amd.ModSpectral(0)
    bc = np.load(os.path.join(os.path.dirname(pyspeedy_amd.__file__), "data", "example_bc.npz"))
    model = EnsembleModel(sp, args.members)
    model.init_sst_anom(args.days // 28 + 2)
    model.set_bc(bc, start_date=(1982, 1, 1, 0, 0))
    model.spectral2grid()
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng(i).normal(0.0, 0.01, (96, 48, 8)).transpose(2, 1, 0) for i in range(args.members)])
    t_grid += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral()

    pw = pyspeedy_amd.projection_weights(sp)
    regions = pw.box(*BOX)[None]
    samples = 4 * args.days
    model.plev_configure([500.0])  # (mslp is the pressure-level kernel's)
    model.tracktape_configure(regions, [("mslp", 0, 0, "min", RADIUS), ("mslp", 0, 0, "min", 0)], EVERY, samples)
    failed, _ = model.run_checked(EVERY * samples)  # one device call for the whole run
    if (failed >= 0).any():
        raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())

    info = model.tracktape_info
    times = model.tracktape_times()
    track = model.tracktape().cpu().numpy()  # [members][samples][2][4]
    assert track.shape == (args.members, samples, 2, 4)
    lon, lat = EnsembleModel.tracktape_lonlat(track)
    print("%d members, %d samples held of %d taken (every %d steps); the low of member 0, followed within %d grid points, and the "
          "deepest point of the box" % (args.members, info["held"], info["taken"], info["every"], RADIUS))
    print("  date                 followed: hPa     lon     lat     deepest: hPa     lon     lat    members whose two differ")
    for s, when in enumerate(times):
        apart = int((track[:, s, 0, 1] != track[:, s, 1, 1]).sum())
        print("  %s  %14.2f %7.2f %7.2f  %14.2f %7.2f %7.2f  %6d" % (
            when.strftime("%Y-%m-%d %H:%M"), 0.01 * track[0, s, 0, 0], lon[0, s, 0], lat[0, s, 0], 0.01 * track[0, s, 1, 0], lon[0, s, 1],
            lat[0, s, 1], apart))
    last = model.tracktape_positions()
    print("where the members' followed lows ended (row, column):", [(int(p) // 96, int(p) % 96) for p in last[:, 0]])
    model.close()


if __name__ == "__main__":
    main()
