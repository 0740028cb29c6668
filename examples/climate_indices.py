#!/usr/bin/env python3
"""Daily climate indices of a perturbed ensemble, formed on the GPU as scalar series.

Every member gets the same boundary fields and a tiny random change of its grid-point temperature (as examples/climate_means.py).
What most studies plot of such a run is not fields but a handful of index series: the global means of the lowest-level temperature
and of precipitation, the Nino-3.4 box mean of the lowest-level temperature, an NAO-like difference of the sea-level pressure of
two boxes, the 500 hPa height at a station.  Each is a fixed weight map applied to one plane of the state, so the projection tape
(EnsembleModel.projtape_*) forms them on the device behind one step a day inside a single multi-day call: eight bytes per member,
index and day come back instead of 18 KB planes.  The weight maps come from pyspeedy_amd.projection_weights (quadrature weights
of the model's Gaussian grid; a station is a bilinear stencil of four weights).  A difference of two boxes is two entries, and the
difference is taken here.

    python examples/climate_indices.py [--members 8] [--days 10]

API surface used: pyspeedy_amd.projection_weights (global_mean, box, point), EnsembleModel.plev_configure, projtape_configure /
projtape_info / projtape_times / projtape_entries / projtape, run_checked, device_view + grid2spectral for the perturbation.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EVERY = 36  # model steps of 40 minutes: one sample a day, at 00:00
LEVELS_HPA = (500.0,)
LOWEST = 7  # the model level next to the ground
# the weight maps: name -> (method of ProjectionWeights, its arguments)
PATTERNS = {
    "global": ("global_mean", ()),
    "nino34": ("box", (190.0, 240.0, -5.0, 5.0)),      # 170 W ... 120 W, 5 S ... 5 N
    "azores": ("box", (-28.0, -10.0, 33.0, 42.0)),     # 28 W ... 10 W, 33 N ... 42 N
    "iceland": ("box", (-25.0, -13.0, 60.0, 70.0)),    # 25 W ... 13 W, 60 N ... 70 N
    "station": ("point", (11.3, 47.9)),                # between grid points, in the Alps
}
# the indices: label, unit, scale, and the entries (name, level, pattern) whose sum the index is
INDICES = (
    ("t_low_global", "K", 1.0, (("t_grid", LOWEST, "global"),)),
    ("precip_global", "mm/day", 1.0, (("precnv", 0, "global"), ("precls", 0, "global"))),
    ("nino34", "K", 1.0, (("t_grid", LOWEST, "nino34"),)),
    ("mslp_azores", "hPa", 0.01, (("mslp", 0, "azores"),)),
    ("mslp_iceland", "hPa", 0.01, (("mslp", 0, "iceland"),)),
    ("z500_station", "m", 1.0, (("z_plev", 0, "station"),)),
)


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])

    def at_least(n):
        def conv(text):
            v = int(text)
            if v < n:
                raise argparse.ArgumentTypeError("must be at least %d" % n)
            return v
        return conv

    p.add_argument("--members", type=at_least(2), default=8, help="ensemble size (the spread needs two)")
    p.add_argument("--days", type=at_least(1), default=10, help="days to simulate: one sample of every index per day")
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
    keys = list(PATTERNS)
    weights = np.stack([getattr(pw, PATTERNS[k][0])(*PATTERNS[k][1]) for k in keys])
    entries, columns = [], []
    for _, _, _, parts in INDICES:
        columns.append(list(range(len(entries), len(entries) + len(parts))))
        entries += [(name, level, keys.index(pattern)) for name, level, pattern in parts]
    model.plev_configure(LEVELS_HPA)
    model.projtape_configure(weights, entries, EVERY, args.days)
    failed, _ = model.run_checked(EVERY * args.days)  # one device call for the whole run
    if (failed >= 0).any():
        raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())

    info = model.projtape_info
    times = model.projtape_times()
    series = model.projtape().cpu().numpy()  # [members][days][entries]
    assert series.shape == (args.members, args.days, len(model.projtape_entries))
    index = {label: scale * series[:, :, cols].sum(axis=2) for (label, _, scale, _), cols in zip(INDICES, columns)}
    index["nao"] = index["mslp_azores"] - index["mslp_iceland"]
    units = {label: unit for label, unit, _, _ in INDICES}
    units["nao"] = "hPa"
    print("%d members, %d samples held of %d taken (every %d steps), %d entries under %d patterns" % (
        args.members, info["held"], info["taken"], info["every"], info["entries"], info["patterns"]))
    shown = ("t_low_global", "precip_global", "nino34", "nao", "z500_station")
    print("  date              " + "".join("%28s" % ("%s [%s]" % (k, units[k])) for k in shown))
    for d, when in enumerate(times):
        cells = "".join("%17.4f +- %8.2e" % (index[k][:, d].mean(), index[k][:, d].std(ddof=1)) for k in shown)
        print("  %s  %s" % (when.strftime("%Y-%m-%d %H:%M"), cells))
    model.close()


if __name__ == "__main__":
    main()
