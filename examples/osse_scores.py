#!/usr/bin/env python3
"""The assimilation experiment of examples/osse_ensrf.py, verified against its truth without leaving the device call.

The nature run is repeated as one more member of the ensemble model: the last member starts unperturbed, the assimilation's mask
leaves it alone, and since members do not depend on their neighbours it is bit for bit the one-member nature run that makes the
observations (asserted at the end).  The verification tape scores the assimilating members against it at every analysis step,
inside the same run_checked() call: RMSE of the ensemble mean, ensemble spread and CRPS of the 850 hPa temperature and the 500 hPa
height over the northern extratropics, the tropics and the southern extratropics -- of the background (the state the analysis
finds) and of the analysis (the state it leaves) -- and the rank histogram of the background.

    python examples/osse_scores.py [--members 20] [--steps 360] [--every 9] [--inflation 1.02] [--seed 0]

API surface used: as examples/osse_ensrf.py, and plev_configure, verif_configure / verif / verif_hist / verif_steps / verif_info.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from osse_ensrf import ENTRIES, SIGMA, SPINUP, parse, weight_maps  # noqa: E402

LEVELS_HPA = (850.0, 500.0)
SCORED = (("T850", "t_plev", 0, "K"), ("Z500", "z_plev", 1, "m"))            # (label, name, level, unit)
REGIONS = (("NH", 20.0, 90.0), ("tropics", -20.0, 20.0), ("SH", -90.0, -20.0))  # (label, lat0, lat1)
SPECTRAL = ("vor", "div", "t", "tr", "ps")


def mask_of(members):
    """member 0 runs freely, the `members` behind it assimilate; the truth, one more member behind them, is left alone as well"""
    mask = np.ones(members + 1, dtype=np.int32)
    mask[0] = 0
    return mask


def score_entries():
    """(name, level, pattern) of the verification tape: every scored field under every region's band"""
    return [(name, level, g) for _, name, level, _ in SCORED for g in range(len(REGIONS))]


def perturb(model, count, seed, std=1.0):
    """a different temperature for each of the first `count` members (examples/osse_ensrf.py); the others are not touched"""
    import torch
    model.spectral2grid(0, count)
    t_grid = model.device_view("t_grid")
    noise = np.stack([np.random.default_rng([seed, i]).normal(0.0, std, (96, 48, 8)).transpose(2, 1, 0) for i in range(count)])
    t_grid[:count] += torch.from_numpy(np.ascontiguousarray(noise)).to(t_grid.device)
    model.grid2spectral(0, count)


def main():
    args = parse()
    import pyspeedy_amd
    from pyspeedy_amd.model import EnsembleModel

    sp = pyspeedy_amd.ModSpectral(0)
    bc = np.load(os.path.join(os.path.dirname(pyspeedy_amd.__file__), "data", "example_bc.npz"))
    pw = pyspeedy_amd.projection_weights(sp)
    maps = weight_maps(pw)
    bands = np.stack([pw.band(lat0, lat1) for _, lat0, lat1 in REGIONS])
    sigma = np.asarray(SIGMA)

    # the nature run on its own: the observations
    nature = EnsembleModel(sp, 1)
    nature.set_bc(bc)
    nature.run(SPINUP)
    nature.projtape_configure(maps, ENTRIES, args.every, max(args.steps // args.every + 1, 1))
    nature.run(args.steps)
    stamps = nature.projtape_steps()
    yo = nature.projtape()[0].cpu().numpy() + sigma * np.random.default_rng([args.seed, 1 << 20]).standard_normal((len(stamps), len(ENTRIES)))

    # the ensemble with the nature run as its last member: analyses and scores on the device between the steps of one call
    truth = args.members + 1
    model = EnsembleModel(sp, args.members + 2)
    model.set_bc(bc)
    perturb(model, args.members + 1, args.seed)
    model.run(SPINUP)
    mask = np.append(mask_of(args.members), 0)
    model.plev_configure(LEVELS_HPA)
    model.assim_configure(maps, ENTRIES, mask, args.every, capacity=max(len(stamps), 1), inflation=args.inflation)
    model.assim_observations(stamps, yo, sigma ** 2)
    model.verif_configure(bands, score_entries(), mask, truth, args.every, capacity=max(len(stamps), 1))
    failed, _ = model.run_checked(args.steps)
    if (failed >= 0).any():
        raise SystemExit("members %s left the accepted range" % np.flatnonzero(failed >= 0).tolist())
    for name in SPECTRAL:  # the truth member IS the nature run
        ours, alone = (np.ascontiguousarray(x).view(np.uint64) for x in (model.get(name, truth), nature.get(name, 0)))
        assert np.array_equal(ours, alone), name
    info = model.verif_info()
    got = {k: v.cpu().numpy() for k, v in model.verif().items()}
    hist = model.verif_hist().cpu().numpy()
    steps = model.verif_steps()
    model.close()
    nature.close()

    done = got["analysis"] == 1
    print("%d members against member %d, scored every %d steps: %d events (steps %d ... %d), an analysis at %d of them" % (
        info["members"], info["truth"], info["every"], len(steps), steps[0], steps[-1], int(done.sum())))
    print("  means over the events with an analysis; b: background, a: analysis")
    print("  field  region    unit   rmse b     rmse a     spread b   spread a   crps b     crps a")
    for k, (label, _, _, unit) in enumerate(SCORED):
        for g, (region, _, _) in enumerate(REGIONS):
            e = k * len(REGIONS) + g
            row = [got[name][done, phase, e].mean() for name in ("rmse", "spread", "crps") for phase in (0, 1)]
            print("  %-6s %-9s %-4s " % (label, region, unit) + " ".join("%10.4g" % v for v in row))
    counts = hist[:, 0, 0, :].sum(axis=0)
    print("  rank histogram of the background, %s %s, all events (%d points; %d ties):" % (SCORED[0][0], REGIONS[0][0], counts.sum(), counts[-1]))
    print("   " + " ".join("%d" % c for c in counts[:-1]))


if __name__ == "__main__":
    main()
